"""trace() frames, probe scenes and the sharded light pass on the multi-device
handle (vrt_lightmap_build_multi, vrt_render_trace_multi[_device],
vrt_trace_frame_multi[_device], vrt_scene_create_multi_probes,
vrt_multi_set_light_mode), on virtual ranks (n replicas on one GPU, the
exchanges done by device copies), a 1-device communicator and, where two GPUs
are visible, a 2-device one.  Bar: bit-exact against the oracle's canonical
order (triangle scenes) or the single-device probe-scene calls that
test_probe_shade_gpu.py pins, for every rank count and both light modes."""
import numpy as np
import pytest
import torch

import pyoracle as po
import voxelraytrace20190722_amd as vrt
from voxelraytrace20190722_amd import _ffi

import cone_path_cases as cc
import probe_cases as pc
from test_probe_scene_gpu import setup_of

pytestmark = pytest.mark.gpu

f32 = np.float32
DEPTH = 5
RANKS = (2, 3, 8)
MODES = ("replicated", "sharded")
LIGHT2 = (vrt.to_radian(60), (-2.0, 9.0, 1.5), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))  # a second light
LFILM = (64, 64)  # the frames' light film
LIGHT_FILMS = [(128, 128), (40, 24), (44, 30)]  # + (16, 16) at n = 8
PROBE_FILM = (48, 36)
LC = (1.0, 0.9, 0.8)


@pytest.fixture(scope="module")
def proxy_small():
    return vrt.SceneData.proxy(0.25, 2)


_handles = {}


@pytest.fixture(scope="module")
def handles(proxy_small):
    """One virtual-rank handle per rank count, shared by the module's tests."""
    def get(n, mode):
        if n not in _handles:
            _handles[n] = vrt.MultiOctree(proxy_small, DEPTH, device_mask=1, virtual_ranks=n)
            assert _handles[n].devices == [0] * n
        _handles[n].light_mode = mode
        return _handles[n]
    yield get
    for m in _handles.values():
        m.close()
    _handles.clear()


_want = {}


def want_lightmap(sd, light, lnx, lny):
    """The oracle's light map: (hits, (key, coverage, illum))."""
    k = ("lm", light, lnx, lny)
    if k not in _want:
        osc, hits = cc.oracle_lightmap(sd, DEPTH, light, lnx, lny)
        _want[k] = (hits, osc.lightmap_nodes())
    return _want[k]


def want_frame(sd, light, lfilm, view, nx, ny, res):
    """The oracle's frame: (image, light hits)."""
    k = ("fr", light, lfilm, view, nx, ny, float(res))
    if k not in _want:
        osc, hits = cc.oracle_lightmap(sd, DEPTH, light, *lfilm)
        _want[k] = (osc.render_trace(po.camera(*view), 1.0, 1.0, nx, ny, res, nthreads=8, samples=False), hits)
    return _want[k]


def rank_shares(sd, light, lnx, lny, n):
    """Each rank's share of the oracle's light hits: the hit samples of the
    tiles that the light film's deal gives the rank."""
    k = ("hit", light, lnx, lny)
    if k not in _want:
        m = po.Scene(sd, DEPTH).ray_march(cc.light_rays(light, lnx, lny))
        _want[k] = (m["hit"] == 1).reshape(lny // 8 * 8, lnx // 8 * 8, 4)
    hit = _want[k]
    rank_of_tile, _ = vrt.tile_deal_map(vrt.Film(1, 1, lnx, lny), n)
    per_tile = hit.reshape(lny // 8, 8, lnx // 8, 8, 4).sum(axis=(1, 3, 4))
    return [int(per_tile[rank_of_tile == r].sum()) for r in range(n)], [int((rank_of_tile == r).sum()) for r in range(n)]


def same_nodes(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(cc.bits(got[1]), cc.bits(want[1]))
            and np.array_equal(cc.bits(got[2]), cc.bits(want[2])))


# ---- the light map -------------------------------------------------------------
@pytest.mark.parametrize("n,lnx,lny", [(n, *f) for n in RANKS for f in LIGHT_FILMS] + [(8, 16, 16)])
def test_lightmap_on_every_rank(proxy_small, handles, n, lnx, lny):
    """128 x 128; 40 x 24: 15 tiles, no whole 4 x 4 block, every tile dealt as a
    leftover; 44 x 30: no multiple of 8; 16 x 16 at n = 8: 4 tiles, so four
    ranks hold no light tile."""
    shares, tiles = rank_shares(proxy_small, cc.LIGHT, lnx, lny, n)
    hits, nodes = want_lightmap(proxy_small, cc.LIGHT, lnx, lny)
    print(f"{lnx} x {lny}, n = {n}: hits per rank {shares}, tiles per rank {tiles}")
    assert sum(shares) == hits and sum(1 for s in shares if s > 0) >= 2
    if (lnx, lny, n) == (16, 16, 8):
        assert sum(1 for t in tiles if t == 0) >= 4 and sum(1 for s in shares if s == 0) >= 1
    cam, film = vrt.Camera(*cc.LIGHT), vrt.Film(1, 1, lnx, lny)
    for mode in MODES:
        m = handles(n, mode)
        assert m.lightmap(cam, film) == hits, mode
        stats = [m.scene(r).lightmap_stats() for r in range(n)]
        for r in range(n):
            assert same_nodes(m.scene(r).lightmap_nodes(), nodes), (mode, r)
        if mode == "sharded":
            assert [s["hits"] for s in stats] == shares
            assert [s["samples"] for s in stats] == [256 * t for t in tiles]
            assert sum(s["hits"] for s in stats) == hits
        else:
            assert [s["hits"] for s in stats] == [hits] * n
            assert [s["samples"] for s in stats] == [256 * sum(tiles)] * n


@pytest.mark.parametrize("n", RANKS)
@pytest.mark.parametrize("mode", MODES)
def test_light_looking_away(proxy_small, handles, n, mode):
    """No hit on any rank: no transfer, no sort, no sums; the light map is all
    coverage and zero illum as the oracle has it, and the frame still renders."""
    hits, nodes = want_lightmap(proxy_small, cc.LIGHT_AWAY, *LFILM)
    assert hits == 0 and not cc.bits(nodes[2]).any() and nodes[1][0] > 0
    m = handles(n, mode)
    # after a lit map, so that nothing of it may remain (both of the scenes' two sets)
    for _ in range(2):
        m.lightmap(vrt.Camera(*cc.LIGHT), vrt.Film(1, 1, *LFILM))
    for _ in range(2):
        assert m.lightmap(vrt.Camera(*cc.LIGHT_AWAY), vrt.Film(1, 1, *LFILM)) == 0
        for r in range(n):
            assert same_nodes(m.scene(r).lightmap_nodes(), nodes), r
            assert m.scene(r).lightmap_stats()["hits"] == 0
    res = m.min_voxel(6)
    nx, ny = cc.FRAME
    want, _ = want_frame(proxy_small, cc.LIGHT_AWAY, LFILM, cc.VIEW, nx, ny, res)
    got, h = m.trace_frame(vrt.Camera(*cc.LIGHT_AWAY), vrt.Film(1, 1, *LFILM), vrt.Camera(*cc.VIEW),
                           vrt.Film(1, 1, nx, ny), res)
    assert h == 0 and cc.same_f32(got, want)


@pytest.mark.parametrize("n", RANKS)
def test_sharded_light_tail(proxy_small, handles, n):
    """VRT_TEST_LIGHT_TAIL: every sample of every rank's share goes through
    k_light_tail, whose work units are the rank's own."""
    hits, nodes = want_lightmap(proxy_small, cc.LIGHT, *LFILM)
    m = handles(n, "sharded")
    vrt.set_test_flags(vrt.TEST_LIGHT_TAIL)
    try:
        assert m.lightmap(vrt.Camera(*cc.LIGHT), vrt.Film(1, 1, *LFILM)) == hits
    finally:
        vrt.set_test_flags(0)
    stats = [m.scene(r).lightmap_stats() for r in range(n)]
    assert all(s["deferred"] == s["samples"] for s in stats)
    assert sum(s["samples"] for s in stats) == 64 * 64 * 4 and sum(s["hits"] for s in stats) == hits
    for r in range(n):
        assert same_nodes(m.scene(r).lightmap_nodes(), nodes), r


# ---- frames ----------------------------------------------------------------------
@pytest.mark.parametrize("n", RANKS)
@pytest.mark.parametrize("mode", MODES)
def test_frames_match_the_oracle(proxy_small, handles, n, mode):
    """40 x 32: one whole block plus a strip, at n = 8 most ranks hold no view
    tile and still take part; 48 x 36: the last four rows stay 0 (the scalar
    unpack path); 4 x 4: no tile at all, the image is zeroed and the light map
    is still built.  min_voxel: the scene's Res (0) and one explicit value."""
    m = handles(n, mode)
    lcam, lfilm = vrt.Camera(*cc.LIGHT), vrt.Film(1, 1, *LFILM)
    res0, res6 = m.min_voxel(0), m.min_voxel(6)
    for nx, ny in [(40, 32), (48, 36)]:
        cam, film = vrt.Camera(*cc.VIEW), vrt.Film(1, 1, nx, ny)
        want, hits = want_frame(proxy_small, cc.LIGHT, LFILM, cc.VIEW, nx, ny, res0)
        got, h = m.trace_frame(lcam, lfilm, cam, film, 0.0)
        assert h == hits and cc.same_f32(got, want), (nx, ny)
        assert np.any(got != 0) and not cc.bits(got[ny // 8 * 8:]).any()
        want6, _ = want_frame(proxy_small, cc.LIGHT, LFILM, cc.VIEW, nx, ny, res6)
        assert not cc.same_f32(want6, want)
        assert m.lightmap(lcam, lfilm) == hits
        assert cc.same_f32(m.render_trace(cam, film, res6), want6), (nx, ny)
        got6, _ = m.trace_frame(lcam, lfilm, cam, film, res6)
        assert cc.same_f32(got6, want6), (nx, ny)
    # no tile: the other light's map is built all the same
    hits2, nodes2 = want_lightmap(proxy_small, LIGHT2, *LFILM)
    got, h = m.trace_frame(vrt.Camera(*LIGHT2), lfilm, vrt.Camera(*cc.VIEW), vrt.Film(1, 1, 4, 4), 0.0)
    assert h == hits2 and got.shape == (4, 4, 3) and not cc.bits(got).any()
    assert hits2 != want_lightmap(proxy_small, cc.LIGHT, *LFILM)[0]
    for r in range(n):
        assert same_nodes(m.scene(r).lightmap_nodes(), nodes2), r
    assert not cc.bits(m.render_trace(vrt.Camera(*cc.VIEW), vrt.Film(1, 1, 4, 4))).any()


@pytest.mark.parametrize("n", RANKS)
@pytest.mark.parametrize("mode", MODES)
def test_buffers_regrow_and_frames_queue_on_one_stream(proxy_small, handles, n, mode):
    """40 x 32 -> 104 x 72 -> 40 x 32 on one handle (the send and gather buffers
    regrow), then three device frames queued on one caller stream without a
    host sync, the light alternating (both trace sets, send buffers reused
    while rank 0 unpacks the previous frame)."""
    m = handles(n, mode)
    res = m.min_voxel(6)
    lfilm = vrt.Film(1, 1, *LFILM)
    for nx, ny in [(40, 32), (104, 72), (40, 32)]:
        want, hits = want_frame(proxy_small, cc.LIGHT, LFILM, cc.VIEW, nx, ny, res)
        got, h = m.trace_frame(vrt.Camera(*cc.LIGHT), lfilm, vrt.Camera(*cc.VIEW), vrt.Film(1, 1, nx, ny), res)
        assert h == hits and cc.same_f32(got, want), (nx, ny)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    queued = []
    for light, (nx, ny) in [(cc.LIGHT, (104, 72)), (LIGHT2, (40, 32)), (cc.LIGHT, (48, 36))]:
        img = torch.full((ny, nx, 3), 7.0, dtype=torch.float32, device="cuda:0")
        h = m.trace_frame_device(vrt.Camera(*light), lfilm, vrt.Camera(*cc.VIEW), vrt.Film(1, 1, nx, ny),
                                 img.data_ptr(), res, stream_ptr=s.cuda_stream)
        queued.append((img, h, light, nx, ny))
    s.synchronize()
    for img, h, light, nx, ny in queued:
        want, hits = want_frame(proxy_small, light, LFILM, cc.VIEW, nx, ny, res)
        assert h == hits and cc.same_f32(img.cpu().numpy(), want), (nx, ny)
    # and the view alone over the last light map, on the caller's stream
    img = torch.full((32, 40, 3), 7.0, dtype=torch.float32, device="cuda:0")
    m.render_trace_device(vrt.Camera(*cc.VIEW), vrt.Film(1, 1, 40, 32), img.data_ptr(), res, s.cuda_stream)
    s.synchronize()
    assert cc.same_f32(img.cpu().numpy(), want_frame(proxy_small, cc.LIGHT, LFILM, cc.VIEW, 40, 32, res)[0])


def test_arguments_on_a_handle(proxy_small):
    m = vrt.MultiOctree(proxy_small, DEPTH, device_mask=1, virtual_ranks=2)
    try:
        L = vrt.lib()
        for mode in (2, -1, 7):
            assert L.vrt_multi_set_light_mode(m.h, mode) == _ffi.VRT_E_INVALID
        with pytest.raises(vrt.VrtError):
            m.light_mode = "striped"
        assert m.light_mode == "replicated"
        m.light_mode = "sharded"
        assert m.light_mode == "sharded"
        cam, film = vrt.Camera(*cc.VIEW), vrt.Film(1, 1, 40, 32)
        with pytest.raises(vrt.VrtError) as e:  # no rank has a light map yet
            m.render_trace(cam, film)
        assert e.value.status == _ffi.VRT_E_INVALID and "no light map" in str(e.value)
        bad = vrt.Film(1, 1, 40, 32)
        bad.c.nx = 0
        lcam, lfilm = vrt.Camera(*cc.LIGHT), vrt.Film(1, 1, *LFILM)
        for call in (lambda: m.trace_frame(lcam, bad, cam, film), lambda: m.trace_frame(lcam, lfilm, cam, bad),
                     lambda: m.lightmap(lcam, bad)):
            with pytest.raises(vrt.VrtError) as e:
                call()
            assert e.value.status == _ffi.VRT_E_INVALID
        assert all(m.scene(r).lightmap_stats()["samples"] == 0 for r in range(2))  # nothing was enqueued
        want, hits = want_frame(proxy_small, cc.LIGHT, LFILM, cc.VIEW, 40, 32, m.min_voxel(6))
        got, h = m.trace_frame(lcam, lfilm, cam, film, m.min_voxel(6))  # the handle stays usable
        assert h == hits and cc.same_f32(got, want)
    finally:
        m.close()


# ---- probe handle -------------------------------------------------------------------
def _probe_arrays(tree):
    return (tree.probe_info(), tree.probe_leaves(), tree.nodes(), tree.leaves())


def _same_arrays(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same_arrays(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                     b.view(np.uint32) if b.dtype == np.float32 else b)
    return a == b


@pytest.mark.parametrize("on_device", [False, True])
def test_probe_handle_replicas_equal_the_single_scene(on_device):
    s = setup_of("proxy", 6)
    single = vrt.VoxelOctree(s.sd, 6, probes=s.probes, build_on_device=on_device)
    m = vrt.MultiOctree(s.sd, 6, device_mask=1, virtual_ranks=3, probes=s.probes, build_on_device=on_device)
    try:
        want = _probe_arrays(single)
        assert want[0][0] == len(s.probes) and want[0][1] > 0
        for r in range(3):
            assert _same_arrays(_probe_arrays(m.scene(r)), want), r
            sg = m.scene(r).probe_sgs
            assert sg["a"].shape == (len(s.probes), 14, 3) and not any(pc.bits(sg[k]).any() for k in sg)
    finally:
        m.close()
        single.close()


@pytest.mark.parametrize("n", RANKS)
@pytest.mark.parametrize("mode", MODES)
def test_probe_handle_frames(n, mode):
    """trace_frame with a light colour equals vrt_trace_frame_probes_device on
    the single scene (pinned by test_probe_shade_gpu.py), on a view with
    triangle hits, probe hits and misses; every rank ends with the single
    scene's SGs; without a light colour the SGs that were set are used."""
    s = setup_of("proxy", 6)
    nx, ny = PROBE_FILM
    light, lfilm = vrt.Camera(*pc.LIGHT), vrt.Film(1, 1, pc.LIGHT_N, pc.LIGHT_N)
    cam, film = vrt.Camera(*cc.VIEW), vrt.Film(1, 1, nx, ny)
    single = vrt.VoxelOctree(s.sd, 6, probes=s.probes)
    m = vrt.MultiOctree(s.sd, 6, device_mask=1, virtual_ranks=n, probes=s.probes, light_mode=mode)
    try:
        res = single.min_voxel(0)

        def single_frame(lc):  # (the single scene leaves the rows below the tile grid as they are)
            img = torch.zeros((ny, nx, 3), dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            h = single.trace_frame_probes_device(light, lfilm, lc, cam, film, 0, 1, 1, img.data_ptr(), res)
            torch.cuda.synchronize()
            return img.cpu().numpy(), h
        want, hits = single_frame(LC)
        _, so = single.render_trace_probes(cam, film, res, samples=True)
        kinds = so["hit"][:nx * (ny // 8 * 8) * 4]
        assert (kinds == 0).sum() >= 10 and (kinds == 1).sum() >= 100 and (kinds == 2).sum() >= 50
        got, h = m.trace_frame(light, lfilm, cam, film, res, light_color=LC)
        assert h == hits and pc.same_f32(got, want)
        sgs = single.probe_sgs
        assert any(pc.bits(sgs[k]).any() for k in sgs)
        for r in range(n):
            back = m.scene(r).probe_sgs
            for k in sgs:
                assert np.array_equal(pc.bits(back[k]), pc.bits(sgs[k])), (r, k)
        # the view alone over the ranks' maps and SGs
        assert pc.same_f32(m.render_trace(cam, film, res), want)
        # light_color = None keeps the stored SGs: here halved ones, set on every rank
        half = {"a": (sgs["a"] * f32(0.5)).astype(f32), "d": sgs["d"], "s": sgs["s"]}
        single.probe_sgs = half
        m.probe_sgs = half
        want_half, _ = single_frame(None)
        assert not pc.same_f32(want_half, want)
        got, h = m.trace_frame(light, lfilm, cam, film, res)
        assert h == hits and pc.same_f32(got, want_half)
        for r in range(n):
            back = m.scene(r).probe_sgs
            for k in half:
                assert np.array_equal(pc.bits(back[k]), pc.bits(half[k])), (r, k)
    finally:
        m.close()
        single.close()


# ---- device counts ---------------------------------------------------------------------
def test_one_rank_real_handle_both_modes(proxy_small):
    """device_mask = 1: a 1-device communicator, the whole light film in
    either mode, a 1-rank gather and the unpack."""
    m = vrt.MultiOctree(proxy_small, DEPTH, device_mask=1)
    try:
        assert m.devices == [0]
        res = m.min_voxel(6)
        nx, ny = 48, 36
        want, hits = want_frame(proxy_small, cc.LIGHT, LFILM, cc.VIEW, nx, ny, res)
        _, nodes = want_lightmap(proxy_small, cc.LIGHT, *LFILM)
        for mode in MODES:
            m.light_mode = mode
            got, h = m.trace_frame(vrt.Camera(*cc.LIGHT), vrt.Film(1, 1, *LFILM), vrt.Camera(*cc.VIEW),
                                   vrt.Film(1, 1, nx, ny), res)
            assert h == hits and cc.same_f32(got, want), mode
            assert same_nodes(m.scene(0).lightmap_nodes(), nodes)
            assert m.scene(0).lightmap_stats()["samples"] == 64 * 64 * 4
    finally:
        m.close()


def test_two_device_handle_both_modes(proxy_small):
    """A real 2-device handle (device_mask 0b11): the gather and, in sharded
    mode, the hit lists' exchange through RCCL.  Skipped on a one-GPU box."""
    if torch.cuda.device_count() < 2:
        pytest.skip("fewer than 2 devices visible")
    m = vrt.MultiOctree(proxy_small, DEPTH, device_mask=0b11)
    try:
        assert m.devices == [0, 1]
        res = m.min_voxel(6)
        _, nodes = want_lightmap(proxy_small, cc.LIGHT, *LFILM)
        for mode in MODES:
            m.light_mode = mode
            for nx, ny in [(104, 72), (40, 32)]:
                want, hits = want_frame(proxy_small, cc.LIGHT, LFILM, cc.VIEW, nx, ny, res)
                got, h = m.trace_frame(vrt.Camera(*cc.LIGHT), vrt.Film(1, 1, *LFILM), vrt.Camera(*cc.VIEW),
                                       vrt.Film(1, 1, nx, ny), res)
                assert h == hits and cc.same_f32(got, want), (mode, nx, ny)
            for r in range(2):
                assert same_nodes(m.scene(r).lightmap_nodes(), nodes), (mode, r)
    finally:
        m.close()
