"""Several lights in one light map on the multi-device handle
(vrt_lightmap_build_lights_multi, vrt_trace_frame_lights_multi[_device]) on
three virtual ranks of one GPU, in both light modes: every rank ends with the
single-device light map of test_lights_gpu.py (the model's) and the frames are
the single scene's, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import voxelraytrace20190722_amd as vrt
from voxelraytrace20190722_amd import _ffi, api

import cone_path_cases as cc
import probe_cases as pc
from test_lights_gpu import FRAME, LC, MA, MB, MC, model, same_nodes, scene, vl
from test_probe_scene_gpu import setup_of

pytestmark = pytest.mark.gpu

DEPTH = 4
N = 3
MODES = ("replicated", "sharded")


@pytest.fixture(scope="module")
def handle():
    sd = scene(DEPTH)[0]
    m = vrt.MultiOctree(sd, DEPTH, device_mask=1, virtual_ranks=N)
    assert m.devices == [0] * N
    yield m
    m.close()


def single_frame(tree, lights, res, lc=None):
    img = torch.zeros((FRAME[1], FRAME[0], 3), device="cuda")
    torch.cuda.synchronize()
    h = tree.trace_frame_lights_device(lights, vrt.Camera(*cc.VIEW), vrt.Film(1, 1, *FRAME), 0, 1, 1, img.data_ptr(),
                                       res, probe_light_color=lc)
    torch.cuda.synchronize()
    return img.cpu().numpy(), h


def test_lightmap_on_every_rank_in_both_modes(handle):
    hits, nodes = model(DEPTH, [MA, MB, MC])
    lights = [vl(MA), vl(MB), vl(MC)]
    tiles = [[int((vrt.tile_deal_map(l.film, N)[0] == r).sum()) for l in lights] for r in range(N)]
    for mode in MODES:
        handle.light_mode = mode
        assert handle.lightmap_lights(lights) == hits == 1353 + 1021 + 2766, mode
        stats = [handle.scene(r).lightmap_stats() for r in range(N)]
        for r in range(N):
            assert same_nodes(handle.scene(r).lightmap_nodes(), nodes), (mode, r)
        if mode == "sharded":  # each rank its tiles of every film's own deal
            assert [s["samples"] for s in stats] == [256 * sum(t) for t in tiles]
            assert sum(s["hits"] for s in stats) == hits and sum(1 for s in stats if s["hits"] > 0) >= 2
        else:
            assert [s["hits"] for s in stats] == [hits] * N
            assert [s["samples"] for s in stats] == [256 * sum(sum(t) for t in tiles)] * N


def test_frames_in_both_modes(handle):
    _, tree, _, _ = scene(DEPTH)
    lights = [vl(MA), vl(MB), vl(MC)]
    res = tree.min_voxel(0)
    want, hits = single_frame(tree, lights, res)
    assert cc.bits(want).any()
    cam, film = vrt.Camera(*cc.VIEW), vrt.Film(1, 1, *FRAME)
    for mode in MODES:
        handle.light_mode = mode
        handle.lightmap_lights([vl(MB)])  # another map first
        got, h = handle.trace_frame_lights(lights, cam, film, res)
        assert h == hits and cc.same_f32(got, want), mode
        handle.lightmap_lights([vl(MB)])
        img = torch.zeros((FRAME[1], FRAME[0], 3), device="cuda")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        assert handle.trace_frame_lights_device(lights, cam, film, img.data_ptr(), res,
                                                stream_ptr=st.cuda_stream) == hits
        st.synchronize()
        assert cc.same_f32(img.cpu().numpy(), want), mode
        # the view alone over the ranks' maps
        assert cc.same_f32(handle.render_trace(cam, film, res), want), mode


def test_a_refusal_enqueues_nothing(handle):
    hits, nodes = model(DEPTH, [MA, MB])
    lights = [vl(MA), vl(MB)]
    assert handle.lightmap_lights(lights) == hits
    before = [handle.scene(r).lightmap_stats() for r in range(N)]
    L = vrt.lib()
    arr, _ = api._lights_arg(lights)
    cam, film = vrt.Camera(*cc.VIEW), vrt.Film(1, 1, *FRAME)
    rgb = np.zeros((FRAME[1], FRAME[0], 3), np.float32)
    p = rgb.ctypes.data_as(_ffi.f32p)
    for a, n in [(arr, 0), (arr, 17), (None, 2)]:
        assert L.vrt_lightmap_build_lights_multi(handle.h, a, n, None) == _ffi.VRT_E_INVALID
        assert L.vrt_trace_frame_lights_multi(handle.h, a, n, None, C.byref(cam.c), C.byref(film.c), 0.0, p,
                                              None) == _ffi.VRT_E_INVALID
    with pytest.raises(vrt.VrtError) as e:
        handle.lightmap_lights([])
    assert e.value.status == _ffi.VRT_E_INVALID
    assert [handle.scene(r).lightmap_stats() for r in range(N)] == before
    for r in range(N):
        assert same_nodes(handle.scene(r).lightmap_nodes(), nodes), r
    assert handle.lightmap_lights(lights) == hits  # the handle stays usable


@pytest.mark.parametrize("mode", MODES)
def test_probe_handle_frame(mode):
    s = setup_of("proxy", DEPTH)
    lights = [vl(MA), vl(MB)]
    single = vrt.VoxelOctree(s.sd, DEPTH, probes=s.inside)
    m = vrt.MultiOctree(s.sd, DEPTH, device_mask=1, virtual_ranks=N, probes=s.inside, light_mode=mode)
    try:
        res = single.min_voxel(0)
        want, hits = single_frame(single, lights, res, LC)
        assert hits == 1353 + 1021 and cc.bits(want).any()
        got, h = m.trace_frame_lights(lights, vrt.Camera(*cc.VIEW), vrt.Film(1, 1, *FRAME), res,
                                      probe_light_color=LC)
        assert h == hits and pc.same_f32(got, want)
        sgs = single.probe_sgs
        assert any(pc.bits(sgs[k]).any() for k in sgs)
        nodes = single.lightmap_nodes()
        for r in range(N):
            back = m.scene(r).probe_sgs
            for k in sgs:
                assert np.array_equal(pc.bits(back[k]), pc.bits(sgs[k])), (r, k)
            assert same_nodes(m.scene(r).lightmap_nodes(), nodes), r
    finally:
        m.close()
        single.close()
