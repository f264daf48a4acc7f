"""VRT_BUILD_DEVICE | VRT_BUILD_DEVICE_PROBES: a probe scene built on the GPU
(vrt_build.hip: the probe frontier beside the triangles') against the host
build of the same scene, array for array, against the float32 restatement of
tests/probe_scene_cases.py, and in use (even_invisible march, trace()).  Bar:
bit-exact."""
import ctypes as C
import os

import numpy as np
import pytest

import voxelraytrace20190722_amd as vrt
from voxelraytrace20190722_amd import _ffi

import probe_cases as pc
import probe_scene_cases as psc
from test_probe_scene_host import _create, probe_set

pytestmark = pytest.mark.gpu

f32 = np.float32
LEAF = np.uint32(0x80000000)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INFO = ("nodes", "internal", "leaves", "nonempty_leaves", "tri_refs")


def scene(name):
    if name == "proxy":
        return vrt.SceneData.proxy(0.25, 2)
    z = np.load(os.path.join(GOLDEN, "scene_soup.npz"), allow_pickle=False)
    return vrt.SceneData(z["pos"], z["nrm"], z["uv"], z["mat"], z["mat_tex"], z["mat_kd"], z["tex_dims"],
                         z["tex_off"], z["tex_data"])


_scenes = {}


def scene_of(name):
    if name not in _scenes:
        sd = scene(name)
        _scenes[name] = (sd, probe_set(sd))
    return _scenes[name]


def same_tree(h, g):
    """Every array of the build: nodes (bits of box, a, b), both kinds of leaf
    lists, the counts and the root box."""
    for x, y in zip(h.nodes(), g.nodes()):
        assert np.array_equal(pc.bits(x), pc.bits(y))
    for x, y in zip(h.leaves(), g.leaves()):
        assert np.array_equal(x, y)
    for x, y in zip(h.probe_leaves(), g.probe_leaves()):
        assert np.array_equal(x, y)
    assert h.probe_info() == g.probe_info()
    assert np.array_equal(pc.bits(np.concatenate(h.root_box)), pc.bits(np.concatenate(g.root_box)))
    for f in INFO:
        assert getattr(h.info, f) == getattr(g.info, f), f


def both(sd, depth, probes):
    """(host build, device build) of one probe scene; the host one stays off
    the device."""
    h = vrt.VoxelOctree(sd, depth, device=-1, probes=probes)
    g = vrt.VoxelOctree(sd, depth, probes=probes, build_on_device=True)
    assert g.info.build_device_ms > 0 and h.info.build_device_ms == 0
    return h, g


def same_march(sd, depth, probes, g, rays):
    """The device-built scene marches like the host-built one, probes
    included: the probe masks of the internal nodes are read here."""
    h = vrt.VoxelOctree(sd, depth, probes=probes)
    a, b = h.ray_march(rays, even_invisible=True), g.ray_march(rays, even_invisible=True)
    for k in a:
        assert np.array_equal(pc.bits(a[k]) if a[k].dtype == np.float32 else a[k],
                              pc.bits(b[k]) if b[k].dtype == np.float32 else b[k]), k
    return b


def aimed_rays(probes, n, seed, spread=0.5):
    """n rays from outside the probes with r > 0, aimed at points within
    spread * r of their centres, the probes taken in turn."""
    rng = np.random.default_rng(seed)
    live = probes[probes[:, 3] > 0]
    rays = []
    for i in range(n):
        p = live[i % len(live)].astype(np.float64)
        d = rng.normal(0, 1, 3)
        d /= np.linalg.norm(d)
        e = rng.normal(0, 1, 3)
        e /= np.linalg.norm(e)
        o = p[:3] + d * p[3] * rng.uniform(1.3, 2.5)
        rays.append(vrt.make_ray(o, p[:3] + e * p[3] * spread * rng.uniform(0, 1) - o))
    return np.array(rays, np.float32)


# ---- 1. device build == host build ---------------------------------------------
@pytest.mark.parametrize("depth", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("name", ["soup", "proxy"])
def test_device_probe_build_equals_host_build(name, depth):
    sd, probes = scene_of(name)
    h, g = both(sd, depth, probes)
    same_tree(h, g)
    n, nl, nr = g.probe_info()
    assert n == len(probes) and nl >= 1 and nr >= 6  # every probe with r > 0 is listed somewhere
    listed = set(g.probe_leaves()[2].tolist())
    assert listed == {0, 1, 2, 3, 4, 5}
    tmx = np.asarray(sd.pos, np.float32).reshape(-1, 3).max(axis=0)
    assert np.all(g.root_box[1] > tmx)  # probe 5 enlarged the root
    if depth == 1:
        # the root is the leaf: every overlapping probe, in index order
        vox, cnt, pr = g.probe_leaves()
        assert vox.tolist() == [0] and cnt.tolist() == [6] and pr.tolist() == [0, 1, 2, 3, 4, 5]


# ---- 2. independent of the host build: the restated insert() ---------------------
_builds = {}


@pytest.mark.parametrize("depth", [3, 5])
@pytest.mark.parametrize("name", ["soup", "proxy"])
def test_device_probe_build_matches_restated(name, depth):
    sd, probes = scene_of(name)
    if name not in _builds:
        _builds[name] = psc.Build(sd.pos, probes, 5)
    wbox, wa, wtris, wprs, _ = _builds[name].at(depth)
    g = vrt.VoxelOctree(sd, depth, probes=probes, build_on_device=True)
    box, a, tl, pl = psc.tree_lists(g)
    assert g.info.nodes == len(wa) == len(a)
    assert pc.same_f32(box, wbox)
    assert pc.same_f32(np.concatenate(g.root_box), psc.root_box(sd.pos, probes))
    leaf = (wa & LEAF) != 0
    assert np.array_equal((a & LEAF) != 0, leaf)
    assert np.array_equal(a[~leaf], wa[~leaf])
    assert np.array_equal(a[leaf] & ~LEAF, [len(t) for t, lf in zip(wtris, leaf) if lf])  # triangle counts only
    for i in range(len(a)):
        assert np.array_equal(tl[i], wtris[i]), i
        assert np.array_equal(pl[i], wprs[i]), i
    assert g.probe_info() == (len(probes), sum(len(p) > 0 for p in wprs), sum(len(p) for p in wprs))
    assert g.info.nonempty_leaves == sum(len(t) > 0 for t in wtris)
    assert g.info.tri_refs == sum(len(t) for t in wtris)
    if depth == 5:
        assert any(len(p) and not len(t) for t, p in zip(wtris, wprs))  # a probe-only leaf
        assert any(len(p) and len(t) for t, p in zip(wtris, wprs))      # probes and triangles in one leaf


# ---- 3. edge scenes --------------------------------------------------------------
def _restated(sd, probes, depth, g):
    wbox, wa, wtris, wprs, _ = psc.Build(sd.pos, probes, depth).at(depth)
    box, a, tl, pl = psc.tree_lists(g)
    assert len(a) == len(wa) and pc.same_f32(box, wbox)
    assert np.array_equal((a & LEAF) != 0, (wa & LEAF) != 0)
    for i in range(len(a)):
        assert np.array_equal(tl[i], wtris[i]) and np.array_equal(pl[i], wprs[i]), i


@pytest.mark.parametrize("depth", [1, 3, 4])
def test_probes_without_triangles(depth):
    """The root box comes from the probes alone."""
    sd = vrt.SceneData(np.zeros((0, 9), np.float32), np.zeros((0, 9), np.float32))
    probes = np.array([(0, 0, 0, 1), (1.5, 0.25, 0, 0.5), (0.3, -0.2, 0.1, 0)], np.float32)
    h, g = both(sd, depth, probes)
    same_tree(h, g)
    assert pc.same_f32(np.concatenate(g.root_box), [-1, -1, -1, 2, 1, 1])
    assert g.info.tri_refs == 0 and g.probe_info()[1] >= 1
    _restated(sd, probes, depth, g)
    if depth == 1:
        assert [x.tolist() for x in g.probe_leaves()] == [[0], [2], [0, 1]]
    rays = aimed_rays(probes, 200, 3)
    hits = same_march(sd, depth, probes, g, rays)
    assert (hits["hit"] == 1).sum() >= 150 and np.all(hits["tri"][hits["hit"] == 1] >= 0)


def test_two_identical_probes():
    """Both appear in every leaf either reaches, in index order."""
    sd, probes = scene_of("soup")
    twins = np.stack([probes[0], probes[0]])
    h, g = both(sd, 4, twins)
    same_tree(h, g)
    vox, cnt, pr = g.probe_leaves()
    assert len(vox) >= 1 and np.all(cnt == 2) and np.array_equal(pr.reshape(-1, 2), np.tile([0, 1], (len(vox), 1)))
    _restated(sd, twins, 4, g)


def test_one_probe_around_the_scene():
    """A sphere that contains the triangles' box: its own box is the root, it
    reaches every cell of the 4^3 grid, so the full tree of depth 4 exists."""
    sd, _ = scene_of("soup")
    pos = np.asarray(sd.pos, np.float32).reshape(-1, 3)
    c, ext = (pos.min(axis=0) + pos.max(axis=0)) / 2, pos.max(axis=0) - pos.min(axis=0)
    big = np.array([(*c, float(np.linalg.norm(ext)))], np.float32)
    h, g = both(sd, 4, big)
    same_tree(h, g)
    assert (g.info.nodes, g.info.internal, g.info.leaves) == (585, 73, 512)
    assert pc.same_f32(np.concatenate(g.root_box), np.concatenate([big[0, :3] - big[0, 3], big[0, :3] + big[0, 3]]))
    n, nl, nr = g.probe_info()
    assert nl == nr and 8 * 27 <= nl < 512  # the corner cells of the cube lie outside the sphere


def test_only_zero_radius_probes():
    """No probe leaves: the tree is the triangle scene's."""
    sd, probes = scene_of("soup")
    zero = probes[[0, 1, 3]].copy()
    zero[:, 3] = 0
    h, g = both(sd, 4, zero)
    same_tree(h, g)
    assert g.probe_info() == (3, 0, 0)
    plain = vrt.VoxelOctree(sd, 4, build_on_device=True)
    for x, y in zip(plain.nodes(), g.nodes()):
        assert np.array_equal(pc.bits(x), pc.bits(y))
    for x, y in zip(plain.leaves(), g.leaves()):
        assert np.array_equal(x, y)
    rays = aimed_rays(probes, 200, 5)
    hits = same_march(sd, 4, zero, g, rays)
    assert np.all(hits["tri"] < sd.ntri)


def test_depth_11_codes():
    """30-bit node codes in the 62-bit leaf keys: 1,500 small triangles and one
    probe of about 3 leaf cells' radius at the deepest grid."""
    rng = np.random.default_rng(11)
    c = rng.uniform(-1, 1, (1500, 1, 3))
    pos = (c + rng.normal(0, 0.05, (1500, 3, 3))).astype(np.float32).reshape(1500, 9)
    sd = vrt.SceneData(pos, rng.normal(0, 1, (1500, 9)).astype(np.float32))
    p3 = pos.reshape(-1, 3)
    ext = p3.max(axis=0) - p3.min(axis=0)
    cell = float(ext.min()) / 1024
    # in the high corner of the grid: the leaf codes there have their top bits set
    probe = np.array([(*(p3.max(axis=0) - 5.3 * cell), 3 * cell)], np.float32)
    h, g = both(sd, 11, probe)
    same_tree(h, g)
    vox, cnt, pr = g.probe_leaves()
    assert 100 <= len(vox) <= 7 ** 3 and np.all(cnt == 1) and not pr.any()
    assert np.all((vox & 0x3FF) >= 1000) and np.all((vox >> 20) >= 1000)


# ---- 4. the built scene works -----------------------------------------------------
def test_device_built_scene_marches_and_traces():
    sd, probes = scene_of("soup")
    ntri, depth = sd.ntri, 5
    host = vrt.VoxelOctree(sd, depth, probes=probes)
    # 4,000 rays: half aimed at the probes, half from around the scene into it
    aimed = aimed_rays(probes, 2000, 21)
    rng = np.random.default_rng(22)
    mn, mx = host.root_box
    o = rng.uniform(mn - 0.3 * (mx - mn), mx + 0.3 * (mx - mn), (2000, 3))
    t = rng.uniform(mn, mx, (2000, 3))
    rays = np.concatenate([aimed, np.array([vrt.make_ray(a, b - a) for a, b in zip(o, t)], np.float32)])
    # the restatement alone, on the host build's tree, over the first aimed rays
    box, a, tl, pl = psc.tree_lists(host)
    keys = pc.node_keys(a)
    walker = psc.Walker(sd, probes, box, a, tl, pl, (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    NW = 400
    want = walker.batch(rays[:NW])
    on_probe = (want["hit"] == 1) & (want["tri"] >= ntri)
    print(f"restated: {on_probe.sum()} of {NW} aimed rays end on a probe")
    assert on_probe.sum() >= 200

    dev = vrt.VoxelOctree(sd, depth, probes=probes, build_on_device=True)
    same_tree(host, dev)
    light, lfilm = vrt.Camera(*pc.LIGHT), vrt.Film(1, 1, pc.LIGHT_N, pc.LIGHT_N)
    rng = np.random.default_rng(5)
    n = len(probes)
    sgs = {"a": rng.uniform(0, 1, (n, 14, 3)).astype(np.float32),
           "d": pc.normalize(rng.normal(0, 1, (n, 14, 3)).astype(np.float32)),
           "s": rng.uniform(1, 12, (n, 14)).astype(np.float32)}
    out = []
    for tree in (host, dev):
        assert tree.lightmap(light, lfilm) > 0
        tree.probe_sgs = sgs
        out.append((tree.ray_march(rays, even_invisible=True), tree.trace(rays, tree.min_voxel(0))))
    (mh, th), (md, td) = out
    for k in mh:
        assert np.array_equal(pc.bits(mh[k]) if mh[k].dtype == np.float32 else mh[k],
                              pc.bits(md[k]) if md[k].dtype == np.float32 else md[k]), k
    assert np.array_equal(pc.bits(th), pc.bits(td))
    ends = (md["hit"] == 1) & (md["tri"] >= ntri)
    print(f"device build: {ends.sum()} of {len(rays)} rays end on a probe, {(md['hit'] == 1).sum()} hit")
    assert ends.sum() >= 200 and ((md["hit"] == 1) & ~ends).sum() >= 200
    # and it is the restatement's march where that was walked
    for k in ("hit", "tri", "voxel"):
        assert np.array_equal(md[k][:NW], want[k][:NW]), k
    assert pc.same_f32(md["hit_p"][:NW], want["hit_p"][:NW]) and pc.same_f32(md["normal"][:NW], want["normal"][:NW])
    assert np.any(td[ends] > 0)


# ---- 5. Python and the raw ABI ------------------------------------------------------
def test_python_passes_both_flags():
    sd, probes = scene_of("soup")
    g = vrt.VoxelOctree(sd, 5, probes=probes, build_on_device=True)
    h = vrt.VoxelOctree(sd, 5, device=-1, probes=probes)
    same_tree(h, g)
    assert g.info.build_device_ms > 0
    # the same call by hand: flags == VRT_BUILD_DEVICE | VRT_BUILD_DEVICE_PROBES
    L = vrt.lib()
    rc, raw = _create(sd, probes, len(probes), depth=5, device=0,
                      flags=_ffi.VRT_BUILD_DEVICE | _ffi.VRT_BUILD_DEVICE_PROBES)
    assert rc == _ffi.VRT_OK, L.vrt_last_error()
    try:
        info = _ffi.SceneInfo()
        assert L.vrt_scene_info(raw, C.byref(info)) == 0
        assert info.nodes == g.info.nodes and info.build_device_ms > 0
        box, a, b = (np.zeros((info.nodes, 6), np.float32), np.zeros(info.nodes, np.uint32),
                     np.zeros(info.nodes, np.uint32))
        assert L.vrt_scene_nodes(raw, vrt.api.ptr(box, _ffi.f32p), vrt.api.ptr(a, _ffi.u32p),
                                 vrt.api.ptr(b, _ffi.u32p)) == 0
        for x, y in zip(g.nodes(), (box, a, b)):
            assert np.array_equal(pc.bits(x), pc.bits(y))
        n_, nl, nr = C.c_int32(-1), C.c_int64(-1), C.c_int64(-1)
        assert L.vrt_scene_probe_info(raw, C.byref(n_), C.byref(nl), C.byref(nr)) == 0
        assert (n_.value, nl.value, nr.value) == g.probe_info()
    finally:
        L.vrt_scene_destroy(raw)
    # VRT_BUILD_DEVICE alone stays refused, and without probes the Python flag is the triangle build's
    rc, raw = _create(sd, probes, len(probes), depth=5, device=0, flags=_ffi.VRT_BUILD_DEVICE)
    assert rc == _ffi.VRT_E_INVALID and not raw.value
    plain = vrt.VoxelOctree(sd, 5, build_on_device=True)
    assert plain.probe_info() == (0, 0, 0) and plain.info.build_device_ms > 0
