"""Several coloured lights in one light map on the GPU
(vrt_lightmap_build_lights, vrt_trace_frame_lights_device) against the float32
model of tests/lights_model.py, which test_lights_model.py pins to the oracle.
Bar: bit-exact -- hits, node keys, coverage and illum of lightmap_nodes, and
the cone-traced images."""
import ctypes as C

import numpy as np
import pytest
import torch

import pyoracle as po
import voxelraytrace20190722_amd as vrt
from voxelraytrace20190722_amd import _ffi, api

import cone_path_cases as cc
import lights_model as lm
import probe_cases as pc
import probe_scene_cases as psc
from test_probe_scene_gpu import setup_of

pytestmark = pytest.mark.gpu

f32 = np.float32
DEPTHS = (4, 6)
FRAME = (40, 32)
LC = (1.0, 0.9, 0.8)  # a probe gather's miss colour: not a light's colour
MA, MB, MC, MZ = lm.issue_lights(vrt.to_radian)


def vl(m):
    """The library's Light of a model light."""
    return vrt.Light(vrt.Camera(*m.cam), vrt.Film(1, 1, *m.film), m.color)


def same_nodes(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(cc.bits(got[1]), cc.bits(want[1]))
            and np.array_equal(cc.bits(got[2]), cc.bits(want[2])))


_state = {}


def scene(depth):
    """(scene data, device octree, oracle scene, model key) per depth, built once."""
    if depth not in _state:
        sd = vrt.SceneData.proxy(0.25, 2)
        _state[depth] = (sd, vrt.VoxelOctree(sd, depth), po.Scene(sd, depth), ("proxy", depth))
    return _state[depth]


_want = {}


def model(depth, lights):
    """The model's (hits, nodes) for the lights in this order, computed once."""
    k = (depth, tuple((l.cam, l.film, l.color) for l in lights))
    if k not in _want:
        _, _, osc, key = scene(depth)
        _want[k] = lm.lightmap(osc, key, lights)
    return _want[k]


def view_image(tree, probes=False):
    img = torch.zeros((FRAME[1], FRAME[0], 3), device="cuda")
    torch.cuda.synchronize()
    call = tree.render_trace_probes_device if probes else tree.render_trace_device
    call(vrt.Camera(*cc.VIEW), vrt.Film(1, 1, *FRAME), 0, 1, 1, img.data_ptr(), tree.min_voxel(0))
    torch.cuda.synchronize()
    return img.cpu().numpy()


# ---- 1. one white light is vrt_lightmap_build ----------------------------------
@pytest.mark.parametrize("depth", DEPTHS)
def test_one_white_light_is_lightmap_build(depth):
    _, tree, _, _ = scene(depth)
    A = vl(MA)
    want_hits = tree.lightmap(A.camera, A.film)
    want_nodes = tree.lightmap_nodes()
    want_img = tree.render_trace(vrt.Camera(*cc.VIEW), vrt.Film(1, 1, *FRAME))
    tree.lightmap(vrt.Camera(*cc.LIGHT_AWAY), A.film)  # another map in between
    assert tree.lightmap_lights([A]) == want_hits == 1353
    assert same_nodes(tree.lightmap_nodes(), want_nodes)
    assert same_nodes(want_nodes, model(depth, [MA])[1])
    assert cc.same_f32(tree.render_trace(vrt.Camera(*cc.VIEW), vrt.Film(1, 1, *FRAME)), want_img)
    assert cc.bits(want_img).any()


# ---- 2. one coloured light ---------------------------------------------------------
@pytest.mark.parametrize("depth", DEPTHS)
def test_one_coloured_light(depth):
    _, tree, _, _ = scene(depth)
    hits, nodes = model(depth, [MB])
    assert tree.lightmap_lights([vl(MB)]) == hits == 1021
    got = tree.lightmap_nodes()
    assert same_nodes(got, nodes)
    assert tree.lightmap_lights([vl(MB.white())]) == hits
    white = tree.lightmap_nodes()
    assert same_nodes(white, model(depth, [MB.white()])[1])
    assert not np.array_equal(cc.bits(white[2]), cc.bits(got[2]))


# ---- 3. the order of the lights ------------------------------------------------------
@pytest.mark.parametrize("depth", DEPTHS)
def test_order_of_the_lights(depth):
    _, tree, osc, key = scene(depth)
    assert lm.shared_leaves(osc, key, [MA, MB]) >= 50
    assert lm.order_sensitive(osc, key, [MA, MB], [MB, MA]) >= 20
    maps = []
    for order in ([MA, MB], [MB, MA]):
        hits, nodes = model(depth, order)
        assert tree.lightmap_lights([vl(l) for l in order]) == hits == 1353 + 1021
        maps.append(tree.lightmap_nodes())
        assert same_nodes(maps[-1], nodes), [l.film for l in order]
    assert not np.array_equal(cc.bits(maps[0][2]), cc.bits(maps[1][2]))


# ---- 4. odd films ----------------------------------------------------------------------
@pytest.mark.parametrize("depth", DEPTHS)
def test_odd_films(depth):
    """B: 40 x 72, not square; C: 48 x 24; Z: 7 x 64, no tile at all."""
    _, tree, osc, key = scene(depth)
    assert lm.shared_leaves(osc, key, [MA, MB, MC]) >= 50
    assert lm.order_sensitive(osc, key, [MA, MB, MC], [MC, MB, MA]) >= 20
    hits, nodes = model(depth, [MA, MB, MC])
    assert tree.lightmap_lights([vl(MA), vl(MB), vl(MC)]) == hits == 1353 + 1021 + 2766
    assert same_nodes(tree.lightmap_nodes(), nodes)
    assert tree.lightmap_stats()["samples"] == 4 * 64 * (8 * 8 + 5 * 9 + 6 * 3)
    # the reverse order is another map, and the model's
    assert tree.lightmap_lights([vl(MC), vl(MB), vl(MA)]) == hits
    rev = tree.lightmap_nodes()
    assert same_nodes(rev, model(depth, [MC, MB, MA])[1])
    assert not np.array_equal(cc.bits(rev[2]), cc.bits(nodes[2]))
    # a film without a sample: the same status from both calls
    Z = vl(MZ)
    L = vrt.lib()
    rc_one = L.vrt_lightmap_build(tree.h, C.byref(Z.camera.c), C.byref(Z.film.c), None)
    arr, n = api._lights_arg([vl(MA), Z, vl(MB)])
    h = C.c_int64(-1)
    rc_list = L.vrt_lightmap_build_lights(tree.h, arr, n, C.byref(h))
    arr1, _ = api._lights_arg([Z])
    assert L.vrt_lightmap_build_lights(tree.h, arr1, 1, None) == rc_one
    if rc_one == _ffi.VRT_OK:
        assert rc_list == _ffi.VRT_OK and h.value == 1353 + 1021
        assert tree.lightmap_lights([vl(MA), Z, vl(MB)]) == 1353 + 1021
        assert same_nodes(tree.lightmap_nodes(), model(depth, [MA, MB])[1])
    else:
        assert rc_list == rc_one


# ---- 5. the tail walk and the seams between lights ---------------------------------------
@pytest.mark.parametrize("depth", DEPTHS)
def test_every_sample_through_the_tail(depth):
    _, tree, _, _ = scene(depth)
    hits, nodes = model(depth, [MA, MB, MC])
    lights = [vl(MA), vl(MB), vl(MC)]
    total = 4 * 64 * (8 * 8 + 5 * 9 + 6 * 3)
    prev = vrt.test_flags()
    vrt.set_test_flags(prev | vrt.TEST_LIGHT_TAIL)
    try:
        assert tree.lightmap_lights(lights) == hits
        stats = tree.lightmap_stats()
        assert same_nodes(tree.lightmap_nodes(), nodes)
        assert stats["deferred"] == stats["samples"] == total and stats["hits"] == hits
    finally:
        vrt.set_test_flags(prev)
    assert tree.lightmap_lights(lights) == hits
    stats = tree.lightmap_stats()
    assert stats["samples"] == total and stats["hits"] == hits and stats["deferred"] < total
    assert same_nodes(tree.lightmap_nodes(), nodes)


# ---- 6. a probe scene ------------------------------------------------------------------------
@pytest.mark.parametrize("depth", DEPTHS)
def test_probe_scene(depth):
    s = setup_of("proxy", depth)
    _, _, osc, key = scene(depth)
    tree = vrt.VoxelOctree(s.sd, depth, probes=s.inside)
    try:
        _, a, tl, pl = psc.tree_lists(tree)
        keys = pc.node_keys(a)
        nonempty = np.array([len(t) > 0 or len(p) > 0 for t, p in zip(tl, pl)])
        probe_only = np.array([len(t) == 0 and len(p) > 0 for t, p in zip(tl, pl)])
        assert probe_only.sum() >= 1
        hits, want = lm.lightmap(osc, key, [MA, MB], node_keys=np.sort(keys), nonempty_keys=keys[nonempty])
        lights = [vl(MA), vl(MB)]
        assert tree.lightmap_lights(lights) == hits == 1353 + 1021
        got = tree.lightmap_nodes()
        assert same_nodes(got, want)
        assert np.all(got[1][np.searchsorted(got[0], keys[probe_only])] == 1)
        # the frame with a gather = the build, the probes' gather, the view
        res = tree.min_voxel(0)
        sgs = tree.gather_probes(res, LC)
        assert any(pc.bits(sgs[k]).any() for k in sgs)
        want_img = view_image(tree, probes=True)
        tree.probe_sgs = {"a": (sgs["a"] * f32(0.5)).astype(f32), "d": sgs["d"], "s": sgs["s"]}
        tree.lightmap(vrt.Camera(*cc.LIGHT_AWAY), vrt.Film(1, 1, 64, 64))
        img = torch.zeros((FRAME[1], FRAME[0], 3), device="cuda")
        torch.cuda.synchronize()
        h = tree.trace_frame_lights_device(lights, vrt.Camera(*cc.VIEW), vrt.Film(1, 1, *FRAME), 0, 1, 1,
                                           img.data_ptr(), res, probe_light_color=LC)
        torch.cuda.synchronize()
        assert h == hits
        assert cc.same_f32(img.cpu().numpy(), want_img) and cc.bits(want_img).any()
        back = tree.probe_sgs
        for k in sgs:
            assert np.array_equal(pc.bits(back[k]), pc.bits(sgs[k])), k
        assert same_nodes(tree.lightmap_nodes(), want)
    finally:
        tree.close()


# ---- 7. the frame in one call --------------------------------------------------------------------
@pytest.mark.parametrize("depth", DEPTHS)
def test_one_call_frame(depth):
    _, tree, _, _ = scene(depth)
    lights = [vl(MA), vl(MB)]
    hits, nodes = model(depth, [MA, MB])
    cam, film = vrt.Camera(*cc.VIEW), vrt.Film(1, 1, *FRAME)
    res = tree.min_voxel(0)
    assert tree.lightmap_lights(lights) == hits
    want_img = view_image(tree)
    tpr = vrt.tiles_per_rank(film, 3)
    want_tiles = torch.zeros(tpr * 192, device="cuda")
    torch.cuda.synchronize()
    tree.render_trace_device(cam, film, 1, 3, 0, want_tiles.data_ptr(), res)
    torch.cuda.synchronize()
    tree.lightmap(vrt.Camera(*cc.LIGHT_AWAY), vrt.Film(1, 1, 64, 64))  # another map in between
    st = torch.cuda.Stream()
    imgs = [torch.zeros((FRAME[1], FRAME[0], 3), device="cuda") for _ in range(2)]
    tiles = torch.zeros(tpr * 192, device="cuda")
    torch.cuda.synchronize()
    # two frames in a row (they alternate the trace sets), then rank 1 of 3
    for img in imgs:
        assert tree.trace_frame_lights_device(lights, cam, film, 0, 1, 1, img.data_ptr(), res,
                                              stream_ptr=st.cuda_stream) == hits
    assert tree.trace_frame_lights_device(lights, cam, film, 1, 3, 0, tiles.data_ptr(), res,
                                          stream_ptr=st.cuda_stream) == hits
    st.synchronize()
    for img in imgs:
        assert cc.same_f32(img.cpu().numpy(), want_img)
    assert cc.bits(want_img).any()
    assert cc.same_f32(tiles.cpu().numpy(), want_tiles.cpu().numpy()) and cc.bits(want_tiles.cpu().numpy()).any()
    assert same_nodes(tree.lightmap_nodes(), nodes)


# ---- 8. arguments -------------------------------------------------------------------------------------
def test_arguments():
    depth = 4
    _, tree, osc, key = scene(depth)
    L = vrt.lib()
    INV = _ffi.VRT_E_INVALID
    hits, nodes = model(depth, [MA, MB])
    assert tree.lightmap_lights([vl(MA), vl(MB)]) == hits
    want_img = view_image(tree)
    before = tree.lightmap_stats()
    scratch = tree.scratch_bytes()[0]
    A = vl(MA)
    big = vrt.Light(A.camera, vrt.Film(1, 1, 16384, 16384))
    one, _ = api._lights_arg([A])
    seventeen, _ = api._lights_arg([A] * 17)
    two_big, _ = api._lights_arg([big, big])  # 2 x 2^30 samples: above 2^31 - 1
    img = torch.zeros((FRAME[1], FRAME[0], 3), device="cuda")
    cam, film = vrt.Camera(*cc.VIEW), vrt.Film(1, 1, *FRAME)
    refused = [(one, 0), (seventeen, 17), (None, 1), (two_big, 2), (one, -1)]
    for arr, n in refused:
        assert L.vrt_lightmap_build_lights(tree.h, arr, n, None) == INV, n
        assert L.vrt_trace_frame_lights_device(tree.h, arr, n, None, C.byref(cam.c), C.byref(film.c), 0.0, 0, 1, 1,
                                               C.c_void_p(img.data_ptr()), None, None) == INV, n
    assert L.vrt_trace_frame_lights_device(tree.h, one, 1, None, None, C.byref(film.c), 0.0, 0, 1, 1,
                                           C.c_void_p(img.data_ptr()), None, None) == INV
    assert L.vrt_trace_frame_lights_device(tree.h, one, 1, None, C.byref(cam.c), C.byref(film.c), 0.0, 0, 1, 1,
                                           None, None, None) == INV
    # nothing was enqueued or allocated, and the previous map is still current
    assert tree.lightmap_stats() == before and tree.scratch_bytes()[0] == scratch
    assert same_nodes(tree.lightmap_nodes(), nodes)
    assert cc.same_f32(view_image(tree), want_img)
    # the largest list: 16 lights, A's camera, 8 x 8 films, distinct colours
    many = [lm.ModelLight(MA.cam, (8, 8), (0.25 + 0.125 * i, 1.0 - 0.03125 * i, 0.5 + 0.0625 * (i % 5)))
            for i in range(16)]
    mh, mnodes = lm.lightmap(osc, key, many)
    assert mh > 0
    assert tree.lightmap_lights([vl(l) for l in many]) == mh
    assert same_nodes(tree.lightmap_nodes(), mnodes)
    assert tree.lightmap_stats()["samples"] == 16 * 256
