"""Moved, flat and far-cornered scenes (tests/placement_cases.py) on the host:
the host build against the oracle's, and the conditions the GPU comparisons
of tests/test_placement_gpu.py rest on, each asserted on the oracle alone:
enough hits, expansions with more than 4 hit children within reach, and the
chain order's spacing on or off where the placement puts it."""
import numpy as np
import pytest

import pyoracle as po

import placement_cases as plc

CASE_DEPTHS = [(n, d) for n in plc.CASES for d in plc.depths(n)]
FRAMES = [(n, 5) for n in plc.CASES if n not in ("aniso", "far_corner")] + [("t65539", 7), ("t2p20x", 7), ("t1e6", 7),
                                                                            ("far_corner", 4)]
SECONDARY = [("identity", 7), ("t65539", 7), ("t2p20x", 7), ("t1e6", 7), ("far_corner", 4)]


@pytest.mark.parametrize("name,depth", CASE_DEPTHS)
def test_host_build_matches_oracle(name, depth):
    t = plc.host_tree(name, depth)
    info, box = plc.oracle_scene(name, depth).info()
    assert [t.info.nodes, t.info.internal, t.info.leaves, t.info.nonempty_leaves, t.info.tri_refs] == list(info)
    assert np.array_equal(np.concatenate(t.root_box).view(np.uint32), box.view(np.uint32))
    for a, b in zip(t.leaves(), plc.oracle_scene(name, depth).leaves()):
        assert np.array_equal(a, b)


def test_far_corner_and_flat_shapes():
    """far_corner: a root box of +-2e18 and 8 non-empty leaves that each hold
    all 300 triangles; flat: every internal node splits into 8."""
    for depth, nodes in ((2, 9), (4, 137), (6, 265)):
        t = plc.host_tree("far_corner", depth)
        assert t.info.nodes == nodes and t.info.nonempty_leaves == 8
        assert np.all(np.abs(np.concatenate(t.root_box)) >= 2.0 ** 60)
        assert np.all(t.leaves()[1][-8:] >= plc.NTRI)
    t = plc.host_tree("flat", 5)
    assert (t.info.nodes, t.info.leaves, t.info.nonempty_leaves, t.info.tri_refs) == (4681, 4096, 3840, 15680)
    assert plc.host_tree("flat", 6).info.nodes == 35401
    assert plc.degenerate(t.nodes())[:, 1].sum() == t.info.internal


@pytest.mark.parametrize("name,depth", CASE_DEPTHS)
def test_family_a_hits_floor(name, depth):
    """>= 250 oracle hits of family A's 2,000 rays (measured minimum 317)."""
    rays, _ = plc.family(name, depth, "A")
    assert len(rays) == 2000 and len(plc.family(name, depth, "B")[0]) >= 600 and len(plc.family(name, depth, "C")[0]) >= 400
    hits = int(plc.oracle_march(name, depth)["hit"][:2000].sum())
    print(name, depth, "family A oracle hits", hits)
    assert hits >= 250


def test_family_c_is_in_plane():
    """Family C's first half: d_k exactly 0 on an axis whose origin coordinate
    is one of the aimed node's plane coordinates."""
    for name, depth in (("flat", 5), ("t1e6", 7), ("identity", 5)):
        rays, node = plc.family(name, depth, "C")
        box = plc.host_tree(name, depth).nodes()[0]
        for ray, n in zip(rays[:200], node[:200]):
            pl = np.stack(plc.planes(box[n, :3], box[n, 3:]), axis=-1)
            assert any(ray[3 + k] == 0 and ray[k] in pl[k] for k in range(3))
        assert np.all(np.sum(rays[200:, 3:6] == 0, axis=1) == 2)  # axis-parallel


@pytest.mark.parametrize("name,depth", FRAMES)
def test_frame_hits_floor(name, depth):
    """>= 1,000 hit samples of the 48 x 48 frame's 9,216 (measured minimum
    1,257: far_corner; 1,472: flat)."""
    osc = plc.oracle_scene(name, depth)
    fov, eye, spot, up = plc.view(name, plc.host_tree(name, depth))
    _, so = osc.render(po.camera(fov, eye, spot, up), 1.0, 1.0, 48, 48, film_index=1, nthreads=8)
    print(name, depth, "frame hit samples", int(so["hit"].sum()))
    assert so["hit"].sum() >= 1000


@pytest.mark.parametrize("name,depth", SECONDARY)
def test_secondary_floor(name, depth):
    """>= 3,000 secondary rays and >= 700 hits on the 40 x 24 film at 17 spp
    (measured minima 3,153 rays: far_corner, and 1,121 hits: t2p20x)."""
    osc = plc.oracle_scene(name, depth)
    fov, eye, spot, up = plc.view(name, plc.host_tree(name, depth))
    _, rays, d = osc.render_secondary(po.camera(fov, eye, spot, up), 1.0, 1.0, 40, 24, spp=17)
    print(name, depth, "secondary rays", rays, "hits", int(d["hit"].sum()))
    assert rays >= 3000 and d["hit"].sum() >= 700


@pytest.mark.parametrize("name,depth,fam,floor", [("flat", 5, "B", 100), ("flat", 5, "C", 50),
                                                  ("t1e6", 7, "B", 209), ("t1e6", 7, "C", 50),
                                                  ("t2p20x", 7, "B", 131), ("t2p20x", 7, "C", 50)])
def test_more_than_4_hit_children_within_reach(name, depth, fam, floor):
    """(ray, aimed node) pairs whose expansion hits more than 4 children
    (rank_order8), by po.aabb_isect on the child boxes split() makes.
    Measured on the oracle: flat depth 5 B 200, C 100; t1e6 depth 7 B 419,
    C 100; t2p20x depth 7 B 263, C 100.  The floor is half of that, 50 at the
    least.  B's pairs come from the diagonal third and, on the moved scenes,
    from targets that the coarse ulp rounds onto planes; C's are the rays that
    start at a node's (b_x, b_y, b_z)."""
    got = plc.many_hit_pairs(name, depth, fam)
    print(name, depth, fam, "pairs with more than 4 hit children", got)
    assert got >= floor


def test_spacing_on_and_off():
    """restated_wmin per axis: zero on x only for t2p20x and t1e6 at depth 7
    (which turns the whole scene's chain order off), positive on every axis
    for the others; quantised but on for t65539 depth 7 and t1e6 depth 5."""
    f32 = np.float32
    for name in ("t2p20x", "t1e6"):
        nodes = plc.host_tree(name, 7).nodes()
        w = plc.restated_wmin(nodes, per_axis=True)
        assert w[0] == 0 and w[1] > 0 and w[2] > 0, (name, w)
        assert np.all(plc.restated_wmin(nodes) == 0)
    w = plc.restated_wmin(plc.host_tree("t2p20x", 7).nodes(), per_axis=True)
    assert abs(float(w[1]) - 0.03504) < 5e-6 and abs(float(w[2]) - 0.03564) < 5e-6, w
    w = plc.restated_wmin(plc.host_tree("t1e6", 7).nodes(), per_axis=True)
    assert np.array_equal(w, f32([0, 0.03125, 0.03125])), w
    for name, depth in [(n, d) for n in ("identity", "t1024", "t65539", "pi", "aniso") for d in (3, 5, 7)] + [("t1e6", 5)]:
        nodes = plc.host_tree(name, depth).nodes()
        w = plc.restated_wmin(nodes)
        assert np.all(w > 0) and np.array_equal(w, plc.restated_wmin(nodes, per_axis=True)), (name, depth, w)
    assert np.array_equal(plc.restated_wmin(plc.host_tree("t65539", 7).nodes()), f32([0.03125] * 3))
    assert np.array_equal(plc.restated_wmin(plc.host_tree("t1e6", 5).nodes()), f32([0.125, 0.125, 0.140625]))
    # the root box rules: flat has no width on y, far_corner is beyond 2^60
    for name, depth in (("flat", 5), ("far_corner", 4)):
        assert np.all(plc.restated_wmin(plc.host_tree(name, depth).nodes()) == 0)
    # the degenerate nodes the issue counts
    for name, count, of in (("t2p20x", 3820, 4457), ("t1e6", 2319, 4306)):
        t = plc.host_tree(name, 7)
        assert (int(plc.degenerate(t.nodes())[:, 0].sum()), t.info.internal) == (count, of)
