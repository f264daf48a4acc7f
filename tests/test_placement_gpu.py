"""Moved, flat and far-cornered scenes (tests/placement_cases.py) on the GPU:
the device build, the batched march, primary frames, config-5 secondary rays,
the light map and trace(), each against the oracle's literal restatement, and
a small probe scene against the restatement of tests/probe_scene_cases.py.
What the hot path derives from the root box in float arithmetic (child boxes,
child centres and ord_wmin, the enlarged boxes, fast_ok, the cone descent's
cells, the device build's node boxes) rounds differently under these
placements.  Bar: every comparison is on bits, NaN equal to NaN."""
import numpy as np
import pytest

import pyoracle as po
import voxelraytrace20190722_amd as vrt

import placement_cases as plc
import probe_cases as pc
import probe_scene_cases as psc

pytestmark = pytest.mark.gpu

CASE_DEPTHS = [(n, d) for n in plc.CASES for d in plc.depths(n)]
FRAMES = [(n, 5) for n in plc.CASES if n not in ("aniso", "far_corner")] + [("t65539", 7), ("t2p20x", 7), ("t1e6", 7),
                                                                            ("far_corner", 4)]
SECONDARY = [("identity", 7), ("t65539", 7), ("t2p20x", 7), ("t1e6", 7), ("far_corner", 4)]
LIGHT_POSE = 0  # of 16, of the case's own box: the oracle hits 3,702 (flat) .. 8,872 (identity) of 16,384 samples
INFO = ("nodes", "internal", "leaves", "nonempty_leaves", "tri_refs")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_f32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((np.isnan(a) & np.isnan(b)) | (bits(a) == bits(b))))


def _same_hits(got, want):
    for k in ("hit", "tri", "voxel"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("hit_p", "normal"):
        assert _same_f32(got[k], want[k]), k


def _same_tree(h, g):
    for x, y in zip(h.nodes(), g.nodes()):
        assert np.array_equal(bits(x), bits(y))
    for x, y in zip(h.leaves(), g.leaves()):
        assert np.array_equal(x, y)
    for f in INFO:
        assert getattr(h.info, f) == getattr(g.info, f), f
    assert np.array_equal(bits(np.concatenate(h.root_box)), bits(np.concatenate(g.root_box)))


# ---- 1. build -------------------------------------------------------------------
@pytest.mark.parametrize("name,depth", CASE_DEPTHS)
def test_device_build_equals_host_build(name, depth):
    h = plc.host_tree(name, depth)
    g = vrt.VoxelOctree(plc.scene(name), depth, build_on_device=True)
    _same_tree(h, g)
    assert g.info.build_device_ms > 0
    want = plc.restated_wmin(h.nodes())
    assert np.array_equal(bits(g.chain_spacing), bits(want)), (g.chain_spacing, want)
    assert np.array_equal(bits(vrt.VoxelOctree(plc.scene(name), depth).chain_spacing), bits(want))


def test_wide_leaf_formats_are_covered():
    """far_corner's 8 leaves of 300 records and the moved soup of 1,200
    triangles at depth 3 use the 64-byte records, the deep moved scenes the
    48-byte ones; the moved wide scene builds alike on host and device."""
    fmts = {(n, d): vrt.VoxelOctree(plc.scene(n), d).ref_record_bytes
            for n, d in (("far_corner", 2), ("far_corner", 4), ("far_corner", 6), ("t1e6", 7), ("flat", 5))}
    assert fmts == {("far_corner", 2): 64, ("far_corner", 4): 64, ("far_corner", 6): 64, ("t1e6", 7): 48,
                    ("flat", 5): 48}, fmts
    sd = plc.scene("t1e6", plc.NTRI_WIDE)
    h = plc.host_tree("t1e6", 3, plc.NTRI_WIDE)
    g = vrt.VoxelOctree(sd, 3, build_on_device=True)
    assert g.ref_record_bytes == 64
    _same_tree(h, g)
    osc = plc.oracle_scene("t1e6", 3, plc.NTRI_WIDE)
    rays = plc.rays_random(h, "t1e6")
    want = osc.ray_march(rays)
    assert want["hit"].sum() >= 250
    _same_hits(g.ray_march(rays), want)


# ---- 2. march -------------------------------------------------------------------
@pytest.mark.parametrize("name,depth", CASE_DEPTHS)
def test_march_matches_oracle(name, depth):
    """Families A, B and C on the host-built and the device-built tree, then
    config-5-style rays from the oracle's hit points (tmin = the leaf size)."""
    sd = plc.scene(name)
    rays, want = plc.all_rays(name, depth), plc.oracle_march(name, depth)
    sec = plc.secondary_batch(name, depth)
    want2 = plc.oracle_scene(name, depth).ray_march(sec)
    assert want["hit"][:2000].sum() >= 250 and want2["hit"].sum() >= 100
    for on_device in (False, True):
        tree = vrt.VoxelOctree(sd, depth, build_on_device=on_device)
        _same_hits(tree.ray_march(rays), want)
        _same_hits(tree.ray_march(sec), want2)


# ---- 3. frames ------------------------------------------------------------------
def _frame(name, depth, flags=0):
    import torch
    tree = vrt.VoxelOctree(plc.scene(name), depth)
    fov, eye, spot, up = plc.view(name, tree)
    orgb, oso = plc.oracle_scene(name, depth).render(po.camera(fov, eye, spot, up), 1.0, 1.0, 48, 48, film_index=1,
                                                     nthreads=8)
    assert oso["hit"].sum() >= 1000
    cam, film = vrt.Camera(fov, eye, spot, up), vrt.Film(1, 1, 48, 48)
    vrt.set_test_flags(flags)
    try:
        rgb, so = tree.render(cam, film, samples=True)
        rgb2, so2 = tree.render(cam, film, samples=True, counters=True)
        img = torch.zeros((48, 48, 3), dtype=torch.float32, device="cuda:0")
        tree.render_tiles_device(cam, film, 0, 1, 1, img.data_ptr(), None)  # the production kernels
        torch.cuda.synchronize()
    finally:
        vrt.set_test_flags(0)
    for s in (so, so2):
        for key in ("hit", "tri", "voxel"):
            assert np.array_equal(s[key], oso[key]), key
        assert _same_f32(s["rgb"], oso["rgb"])
    assert np.array_equal(so2["counters"], oso["counters"])
    assert _same_f32(rgb, orgb) and _same_f32(rgb2, orgb)
    assert _same_f32(img.cpu().numpy(), orgb)


@pytest.mark.parametrize("name,depth", FRAMES)
def test_frame_matches_oracle(name, depth):
    _frame(name, depth)


@pytest.mark.parametrize("name,depth", [("t1e6", 7), ("flat", 5)])
def test_frame_general_march_matches_oracle(name, depth):
    """Every unit of the production render deferred (VRT_TEST_FORCE_DEFER):
    the general march on the same frames."""
    _frame(name, depth, vrt.TEST_FORCE_DEFER)


# ---- 4. secondary ---------------------------------------------------------------
@pytest.mark.parametrize("name,depth", SECONDARY)
def test_secondary_matches_oracle(name, depth):
    tree = vrt.VoxelOctree(plc.scene(name), depth)
    fov, eye, spot, up = plc.view(name, tree)
    cam, film = vrt.Camera(fov, eye, spot, up), vrt.Film(1, 1, 40, 24)
    ovis, orays, od = plc.oracle_scene(name, depth).render_secondary(po.camera(fov, eye, spot, up), 1.0, 1.0, 40, 24,
                                                                     spp=17)
    assert orays >= 3000 and od["hit"].sum() >= 700
    vis, rays, d = tree.render_secondary(cam, film, spp=17, ids=True)  # the ordered walk
    assert rays == orays
    for k in ("hit", "tri", "voxel"):
        assert np.array_equal(d[k], od[k]), k
    assert _same_f32(vis, ovis)
    vis_any, rays_any = tree.render_secondary(cam, film, spp=17)  # the occlusion walk and its compaction
    assert rays_any == orays
    assert _same_f32(vis_any, ovis)


# ---- 5. light map and trace -------------------------------------------------------
@pytest.mark.parametrize("name,depth", [("identity", 5), ("t65539", 5), ("t1e6", 5), ("flat", 5), ("t1e6", 6)])
def test_lightmap_and_trace_match_oracle(name, depth):
    """The light is sweep pose 0 of 16 of the case's own box on a 64 x 64
    film: the oracle hits 8,872 (identity), 7,908 (t65539), 5,008 (t1e6) and
    3,702 (flat) of 16,384 samples at depth 5; the floor is 1,000.
    flat stops after the light map and min_voxel: its root box has no height,
    so min_voxel(6) is 0, the cone's first distance is 0 and the reference's
    cone march (dist += step * diam) never advances -- the oracle does not
    return, and there is nothing to compare a trace with."""
    sd = plc.scene(name)
    tree = vrt.VoxelOctree(sd, depth)
    osc = po.Scene(sd, depth)
    light = vrt.sweep_pose(*plc.ray_box(name, tree), LIGHT_POSE, 16)
    ohits = osc.lightmap(po.camera(*light), 1.0, 1.0, 64, 64, nthreads=8)
    assert ohits >= 1000
    assert tree.lightmap(vrt.Camera(*light), vrt.Film(1, 1, 64, 64)) == ohits
    k, cov, ill = tree.lightmap_nodes()
    ok, ocov, oill = osc.lightmap_nodes()
    assert np.array_equal(k, ok)
    assert _same_f32(cov, ocov) and _same_f32(ill, oill)
    res = tree.min_voxel(6)
    assert res == osc.min_voxel(6)
    if name == "flat":
        assert res == 0
        return
    fov, eye, spot, up = plc.view(name, tree)
    rgb, so = tree.render_trace(vrt.Camera(fov, eye, spot, up), vrt.Film(1, 1, 32, 32), res, samples=True)
    orgb, oso = osc.render_trace(po.camera(fov, eye, spot, up), 1.0, 1.0, 32, 32, res, nthreads=8)
    assert oso["hit"].sum() >= 1000
    assert np.array_equal(so["hit"], oso["hit"])
    assert _same_f32(so["rgb"], oso["rgb"]) and _same_f32(rgb, orgb)
    # the batched trace() and cone_trace over family A's first 400 rays
    rays = plc.family(name, depth, "A")[0][:400]
    want_hit = osc.ray_march(rays)
    out, parts = tree.trace(rays, res, parts=True)
    assert _same_f32(out, osc.shade_trace(rays, res))
    _same_hits(parts, want_hit)
    hi = np.flatnonzero(want_hit["hit"] == 1)
    assert len(hi) >= 50
    cone = tree.cone_trace(want_hit["hit_p"][hi], want_hit["normal"][hi], res)
    assert _same_f32(cone, parts["indirect"][hi])
    with np.errstate(all="ignore"):
        assert _same_f32(parts["albedo"][hi] * (cone + parts["direct"][hi]), out[hi])


# ---- 6. probes (small) -------------------------------------------------------------
@pytest.mark.parametrize("name", ["t1e6", "identity"])
def test_probe_scene_build_and_march(name):
    """6 probes of two leaf voxels' radius at oracle hit points, depth 5: the
    host build of the probe scene equals the device build (VRT_BUILD_DEVICE |
    VRT_BUILD_DEVICE_PROBES), and the even_invisible march over family A
    equals the restated walker -- for t1e6 the sphere quadratic at coordinates
    of 1e6."""
    depth, sd, probes = 5, plc.scene(name), plc.probe_set(name, 5)
    h = vrt.VoxelOctree(sd, depth, device=-1, probes=probes)
    g = vrt.VoxelOctree(sd, depth, probes=probes, build_on_device=True)
    _same_tree(h, g)
    assert h.probe_info() == g.probe_info() and g.probe_info()[0] == 6 and g.probe_info()[2] >= 6
    for x, y in zip(h.probe_leaves(), g.probe_leaves()):
        assert np.array_equal(x, y)
    box, a, tl, pl = psc.tree_lists(h)
    keys = pc.node_keys(a)
    rays = plc.family(name, depth, "A")[0]
    want = psc.Walker(sd, probes, box, a, tl, pl, (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)).batch(rays)
    on_probe = (want["hit"] == 1) & (want["tri"] >= sd.ntri)
    print(name, "rays that end on a probe", int(on_probe.sum()), "of", int(want["hit"].sum()), "hits")
    assert on_probe.sum() >= 50 and (want["hit"] == 1).sum() - on_probe.sum() >= 250
    for tree in (g, vrt.VoxelOctree(sd, depth, probes=probes)):
        _same_hits(tree.ray_march(rays, even_invisible=True), want)
