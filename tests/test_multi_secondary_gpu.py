"""Config 5 (the stochastic secondary-ray frame) on the multi-device handle:
vrt_render_secondary_multi[_device] and one rank's packed share with the
share-sized primary pass, vrt_render_secondary_tiles_device.  Virtual ranks (n
replicas on one GPU, the gather done by device copies), a 1-device communicator
and, where two GPUs are visible, a 2-device one.  Bar: every value bit-equal to
the oracle's render_secondary (or, for a probe handle, the single probe scene's)
for every rank count.

The views are sweep poses 6 and 9 of 16 at depth 6: every film below has
primary misses and, for 64 and 17 rays per pixel, partially visible pixels on
every rank that owns a tile (asserted, so that no test passes vacuously)."""
import numpy as np
import pytest
import torch

import pyoracle as po
import voxelraytrace20190722_amd as vrt
from voxelraytrace20190722_amd import _ffi

from test_probe_scene_gpu import setup_of

pytestmark = pytest.mark.gpu

DEPTH = 6
RANKS = (2, 3, 8)
POSES = (6, 9)
# 72 x 40: 9 x 5 tiles, ragged strips dealt tile by tile (23/22 at n = 2, 4/20/21 at n = 3);
# 96 x 64: 32 tiles each at n = 3; 512 x 40: whole 4 x 4 blocks, 40 tiles each at n = 8;
# 16 x 16: 4 tiles, at n = 8 ranks 4..7 hold none
FILMS = [(72, 40), (96, 64), (512, 40), (16, 16)]
SENTINEL = 0x7FC0BEEF  # a NaN no kernel writes


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_f32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def proxy_small():
    return vrt.SceneData.proxy(0.25, 2)


_handles = {}


@pytest.fixture(scope="module")
def handles(proxy_small):
    """One virtual-rank handle per rank count, shared by the module's tests."""
    def get(n):
        if n not in _handles:
            _handles[n] = vrt.MultiOctree(proxy_small, DEPTH, device_mask=1, virtual_ranks=n)
            assert _handles[n].devices == [0] * n
        return _handles[n]
    yield get
    for m in _handles.values():
        m.close()
    _handles.clear()


_state = {}


def pose_of(sd, pose):
    if "box" not in _state:
        _state["box"] = vrt.VoxelOctree(sd, DEPTH, device=-1).root_box
    return vrt.sweep_pose(*_state["box"], pose, 16)


def want_vis(sd, pose, nx, ny, spp):
    """The oracle's (vis, rays), computed once per view."""
    k = ("vis", pose, nx, ny, spp)
    if k not in _state:
        if "osc" not in _state:
            _state["osc"] = po.Scene(sd, DEPTH)
        _state[k] = _state["osc"].render_secondary(po.camera(*pose_of(sd, pose)), 1.0, 1.0, nx, ny, spp=spp,
                                                   nthreads=8, ids=False)
    return _state[k]


def want_rgb(sd, pose, nx, ny):
    k = ("rgb", pose, nx, ny)
    if k not in _state:
        want_vis(sd, pose, 16, 16, 1)  # makes the oracle scene
        _state[k] = _state["osc"].render(po.camera(*pose_of(sd, pose)), 1.0, 1.0, nx, ny, nthreads=8, samples=False)
    return _state[k]


def tiles_of(img, nx, ny):
    """(nty, ntx, 8, 8): the tiles of an (ny, nx) image."""
    return img[:ny // 8 * 8, :nx // 8 * 8].reshape(ny // 8, 8, nx // 8, 8).transpose(0, 2, 1, 3)


def check_inputs(sd, pose, nx, ny, n):
    """What the issue's table states of the films: primary misses, and for 64
    and 17 rays per pixel partially visible pixels on every rank with a tile."""
    rank_of, _ = vrt.tile_deal_map(vrt.Film(1, 1, nx, ny), n)
    area = (nx // 8 * 8) * (ny // 8 * 8)
    for spp in (64, 17):
        vis, rays = want_vis(sd, pose, nx, ny, spp)
        assert (rays - area) % spp == 0 and 0 < (rays - area) // spp < area, (nx, ny, spp)
        t = tiles_of(vis, nx, ny)
        for r in range(n):
            mine = t[rank_of == r]
            assert mine.size == 0 or ((mine > 0) & (mine < 1)).any(), (nx, ny, spp, r)
    return [int((rank_of == r).sum()) for r in range(n)]


def test_the_films_are_what_the_tests_need(proxy_small):
    assert check_inputs(proxy_small, 6, 72, 40, 2) == [23, 22]
    assert check_inputs(proxy_small, 6, 72, 40, 3) == [4, 20, 21]
    assert check_inputs(proxy_small, 6, 96, 64, 3) == [32, 32, 32]
    assert check_inputs(proxy_small, 6, 512, 40, 8) == [40] * 8
    assert check_inputs(proxy_small, 6, 16, 16, 8) == [1, 1, 1, 1, 0, 0, 0, 0]
    area = 72 * 40
    assert [(want_vis(proxy_small, p, 72, 40, 64)[1] - area) // 64 for p in POSES] == [2299, 2339]


# ---- 1. frames -------------------------------------------------------------------
@pytest.mark.parametrize("n", RANKS)
def test_frames_match_the_oracle(proxy_small, handles, n):
    m = handles(n)
    for nx, ny in FILMS:
        for pose in POSES:
            check_inputs(proxy_small, pose, nx, ny, n)
            cam, film = vrt.Camera(*pose_of(proxy_small, pose)), vrt.Film(1, 1, nx, ny)
            for spp in (64, 17, 1):
                want, rays = want_vis(proxy_small, pose, nx, ny, spp)
                got, r = m.render_secondary(cam, film, spp)
                assert r == rays and same_f32(got, want), (nx, ny, pose, spp)
    # no tile: zeros and no ray
    got, r = m.render_secondary(vrt.Camera(*pose_of(proxy_small, 6)), vrt.Film(1, 1, 7, 20), 64)
    assert r == 0 and got.shape == (20, 7) and not bits(got).any()
    assert want_vis(proxy_small, 6, 7, 20, 64)[1] == 0
    img = torch.full((20, 7), 7.0, dtype=torch.float32, device="cuda:0")
    m.render_secondary_device(vrt.Camera(*pose_of(proxy_small, 6)), vrt.Film(1, 1, 7, 20), 64, img.data_ptr())
    assert not bits(img.cpu().numpy()).any()


# ---- 2. every config-5 path -----------------------------------------------------
@pytest.mark.parametrize("flags", [vrt.TEST_SPILL_ALL, vrt.TEST_SPILL_ALL | vrt.TEST_STREAM_LEFTOVER,
                                   vrt.TEST_SEC_DEFER, vrt.TEST_SEC_DEFER | vrt.TEST_SPILL_ALL])
def test_every_secondary_path_through_the_handle(proxy_small, handles, flags):
    """The compaction queue with every ray stopped at its first end, the resume
    launch's leftover chunks, and the deferred pixels' exact walk, on each
    rank's own pixels."""
    m = handles(3)
    nx, ny, pose = 96, 64, 6
    want, rays = want_vis(proxy_small, pose, nx, ny, 64)
    vrt.set_test_flags(flags)
    try:
        got, r = m.render_secondary(vrt.Camera(*pose_of(proxy_small, pose)), vrt.Film(1, 1, nx, ny), 64)
        stats = [m.scene(k).secondary_spill_stats() for k in range(3)]
    finally:
        vrt.set_test_flags(0)
    assert r == rays and same_f32(got, want)
    print(stats)
    if flags & vrt.TEST_SPILL_ALL:  # every wave stops at its first ended ray: each rank queues rays
        assert all(s["records"] > 0 for s in stats), stats
    if flags & vrt.TEST_STREAM_LEFTOVER:
        assert all(s["leftover_chunks"] > 0 for s in stats), stats
    if flags & vrt.TEST_SEC_DEFER:
        assert all(s["deferred_pixels"] > 0 for s in stats), stats


# ---- 3. the primary pass is share-sized ------------------------------------------
@pytest.fixture(scope="module")
def single(proxy_small):
    t = vrt.VoxelOctree(proxy_small, DEPTH)
    yield t
    t.close()


def _sentinel(n):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda:0")


def _share(tree, cam, film, spp, r, n, tpr):
    """vrt_render_secondary_tiles_device over sentinel-filled buffers ->
    (prim words (H8, W8, 8), vis words (ny, nx), packed floats, hits)."""
    nx, ny = film.nx, film.ny
    w8, h8 = nx // 8 * 8, ny // 8 * 8
    prim, vis, packed = _sentinel(max(1, w8 * h8) * 8), _sentinel(nx * ny), _sentinel(max(1, tpr) * 64)
    hits = torch.full((1,), 123456789, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    tree.render_secondary_tiles_device(cam, film, spp, r, n, prim.data_ptr(), vis.data_ptr(), packed.data_ptr(),
                                       hits.data_ptr())
    torch.cuda.synchronize()
    return (prim.cpu().numpy().view(np.uint32)[:w8 * h8 * 8].reshape(h8, w8, 8),
            vis.cpu().numpy().view(np.uint32).reshape(ny, nx), packed.cpu().numpy().view(np.float32),
            int(hits.item()))


def _packed_want(one, film, r, n):
    """Rank r's tiles of the one-rank image in deal order."""
    rank_of, slot_of = vrt.tile_deal_map(film, n)
    t = tiles_of(one, film.nx, film.ny)
    cnt = int((rank_of == r).sum())
    out = np.zeros((cnt, 64), np.float32)
    out[slot_of[rank_of == r]] = t[rank_of == r].reshape(cnt, 64)
    assert sorted(slot_of[rank_of == r]) == list(range(cnt))
    return out.ravel()


@pytest.mark.parametrize("nx,ny,n", [(72, 40, 3), (512, 40, 8), (72, 40, 1)])
def test_primary_pass_is_share_sized(proxy_small, single, nx, ny, n):
    pose, spp = 9, 17
    cam, film = vrt.Camera(*pose_of(proxy_small, pose)), vrt.Film(1, 1, nx, ny)
    one, rays = single.render_secondary(cam, film, spp)
    want, wrays = want_vis(proxy_small, pose, nx, ny, spp)
    assert rays == wrays and same_f32(one, want)
    rank_of, _ = vrt.tile_deal_map(film, n)
    tpr = vrt.lib().vrt_tiles_per_rank(film.c, n)
    own_px = np.kron(rank_of, np.ones((8, 8), np.int32))  # (H8, W8): the pixel's rank
    total = misses = 0
    for r in range(n):
        # the whole-film pass of vrt_render_secondary_device leaves every record
        ref_prim, ref_vis = _sentinel(nx * ny * 8), torch.zeros(nx * ny, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        single.render_secondary_device(cam, film, spp, r, n, ref_prim.data_ptr(), ref_vis.data_ptr())
        torch.cuda.synchronize()
        ref = ref_prim.cpu().numpy().view(np.uint32)[:own_px.size * 8].reshape(*own_px.shape, 8)
        assert not (ref[..., 0] == SENTINEL).any()
        prim, vis, packed, hits = _share(single, cam, film, spp, r, n, tpr)
        mine = own_px == r
        assert mine.any()
        # other ranks' records and pixels: untouched
        assert (prim[~mine] == SENTINEL).all()
        assert (vis[:own_px.shape[0], :own_px.shape[1]][~mine] == SENTINEL).all()
        assert (vis[own_px.shape[0]:] == SENTINEL).all() and (vis[:, own_px.shape[1]:] == SENTINEL).all()
        # own records: word 0 always, words 1..6 of a hit
        assert np.array_equal(prim[mine][:, 0], ref[mine][:, 0])
        hit = mine & (ref[..., 0] != 0)
        assert hit.any()
        misses += int((mine & ~hit).sum())
        assert np.array_equal(prim[hit][:, :7], ref[hit][:, :7])
        assert hits == int(hit.sum())
        assert np.array_equal(vis[:own_px.shape[0], :own_px.shape[1]][mine],
                              bits(one)[:own_px.shape[0], :own_px.shape[1]][mine])
        cnt = int((rank_of == r).sum())
        assert np.array_equal(bits(packed[:cnt * 64]), bits(_packed_want(one, film, r, n)))
        assert (bits(packed[cnt * 64:]) == SENTINEL).all()
        total += hits
    assert total == (rays - own_px.size) // spp and misses == own_px.size - total > 0


def test_rank_without_a_tile_touches_nothing(proxy_small, single):
    cam, film = vrt.Camera(*pose_of(proxy_small, 6)), vrt.Film(1, 1, 16, 16)
    prim, vis, packed, hits = _share(single, cam, film, 64, 5, 8, 1)
    assert hits == 0
    assert (prim == SENTINEL).all() and (vis == SENTINEL).all() and (bits(packed) == SENTINEL).all()


# ---- 4. the computed deal --------------------------------------------------------
def test_computed_deal_fallback(proxy_small):
    """36 distinct (tile grid, nranks, rank) deals on one scene, every rank with
    a tile: the scene tables 32, the last four are computed by the kernels
    (deal_tile) -- rank 2 of a grid without a whole block, then every rank of
    9 x 5 tiles (whole blocks, the right and the bottom strip)."""
    films = [(64, 40), (56, 40), (48, 40), (40, 40), (72, 32), (56, 32), (48, 32), (40, 32), (48, 24), (40, 24),
             (24, 24), (72, 40)]
    n, spp, pose = 3, 17, 6
    tree = vrt.VoxelOctree(proxy_small, DEPTH)
    try:
        cam = vrt.Camera(*pose_of(proxy_small, pose))
        ones = {}
        for nx, ny in films:
            ones[(nx, ny)], _ = tree.render_secondary(cam, vrt.Film(1, 1, nx, ny), spp)
            assert same_f32(ones[(nx, ny)], want_vis(proxy_small, pose, nx, ny, spp)[0])
        grew = []
        for nx, ny in films:
            film = vrt.Film(1, 1, nx, ny)
            rank_of, _ = vrt.tile_deal_map(film, n)
            tpr = vrt.lib().vrt_tiles_per_rank(film.c, n)
            for r in range(n):
                assert (rank_of == r).any()
                total0, spill0 = tree.scratch_bytes()
                _, _, packed, _ = _share(tree, cam, film, spp, r, n, tpr)
                total1, spill1 = tree.scratch_bytes()
                grew.append((total1 - spill1) - (total0 - spill0))
                cnt = int((rank_of == r).sum())
                assert np.array_equal(bits(packed[:cnt * 64]), bits(_packed_want(ones[(nx, ny)], film, r, n))), \
                    (nx, ny, r)
        # a tabled deal adds its table to the scene's scratch, a computed one nothing
        assert all(g > 0 for g in grew[:32]) and grew[32:] == [0, 0, 0, 0], grew
    finally:
        tree.close()


# ---- 5. mixed frames, regrowth, stream order -----------------------------------------
def test_mixed_frames_regrowth_and_stream_order(proxy_small):
    m = vrt.MultiOctree(proxy_small, DEPTH, device_mask=1, virtual_ranks=3)
    try:
        cam6 = vrt.Camera(*pose_of(proxy_small, 6))

        def primary(nx, ny):
            got = m.render(cam6, vrt.Film(1, 1, nx, ny))
            assert same_f32(got, want_rgb(proxy_small, 6, nx, ny)) and got.any()
        primary(72, 40)
        for nx, ny in [(72, 40), (512, 40)]:  # the second regrows every buffer
            want, rays = want_vis(proxy_small, 6, nx, ny, 64)
            got, r = m.render_secondary(cam6, vrt.Film(1, 1, nx, ny), 64)
            assert r == rays and same_f32(got, want), (nx, ny)
        primary(512, 40)
        primary(72, 40)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        queued = []
        for pose, nx, ny, spp in [(6, 512, 40, 64), (9, 72, 40, 17), (9, 96, 64, 64)]:
            img = torch.full((ny, nx), 7.0, dtype=torch.float32, device="cuda:0")
            m.render_secondary_device(vrt.Camera(*pose_of(proxy_small, pose)), vrt.Film(1, 1, nx, ny), spp,
                                      img.data_ptr(), s.cuda_stream)
            queued.append((img, pose, nx, ny, spp))
        s.synchronize()
        for img, pose, nx, ny, spp in queued:
            assert same_f32(img.cpu().numpy(), want_vis(proxy_small, pose, nx, ny, spp)[0]), (pose, nx, ny, spp)
        # and a host frame behind them gets its own hit count
        want, rays = want_vis(proxy_small, 9, 72, 40, 64)
        got, r = m.render_secondary(vrt.Camera(*pose_of(proxy_small, 9)), vrt.Film(1, 1, 72, 40), 64)
        assert r == rays and same_f32(got, want)
    finally:
        m.close()


# ---- 6. other handles ------------------------------------------------------------------
def test_probe_handle_skips_the_probes():
    s = setup_of("proxy", 6)
    single = vrt.VoxelOctree(s.sd, 6, probes=s.probes)
    m = vrt.MultiOctree(s.sd, 6, device_mask=1, virtual_ranks=2, probes=s.probes)
    try:
        assert single.probe_info()[0] == len(s.probes) > 0
        cam, film = vrt.Camera(*vrt.sweep_pose(*single.root_box, 6, 16)), vrt.Film(1, 1, 72, 40)
        for spp in (64, 17):
            want, rays = single.render_secondary(cam, film, spp)
            assert ((want > 0) & (want < 1)).any() and rays > 72 * 40
            got, r = m.render_secondary(cam, film, spp)
            assert r == rays and same_f32(got, want), spp
    finally:
        m.close()
        single.close()


def test_one_device_communicator(proxy_small):
    """device_mask = 1 without virtual ranks: a 1-rank gather (in place) and
    the unpack; the share-sized pass in raster order."""
    m = vrt.MultiOctree(proxy_small, DEPTH, device_mask=1)
    try:
        assert m.devices == [0]
        for nx, ny, spp in [(72, 40, 64), (96, 64, 17), (7, 20, 64)]:
            want, rays = want_vis(proxy_small, 9, nx, ny, spp)
            got, r = m.render_secondary(vrt.Camera(*pose_of(proxy_small, 9)), vrt.Film(1, 1, nx, ny), spp)
            assert r == rays and same_f32(got, want), (nx, ny, spp)
    finally:
        m.close()


def test_two_device_handle(proxy_small):
    """A real 2-device handle (device_mask 0b11): the gather through RCCL.
    Skipped on a one-GPU box."""
    if torch.cuda.device_count() < 2:
        pytest.skip("fewer than 2 devices visible")
    m = vrt.MultiOctree(proxy_small, DEPTH, device_mask=0b11)
    try:
        assert m.devices == [0, 1]
        for nx, ny, spp in [(72, 40, 64), (512, 40, 17), (72, 40, 1)]:
            want, rays = want_vis(proxy_small, 6, nx, ny, spp)
            got, r = m.render_secondary(vrt.Camera(*pose_of(proxy_small, 6)), vrt.Film(1, 1, nx, ny), spp)
            assert r == rays and same_f32(got, want), (nx, ny, spp)
    finally:
        m.close()


# ---- 7. arguments on a live handle -------------------------------------------------------
def test_arguments_on_a_live_handle(proxy_small, handles):
    import ctypes as C
    m = handles(2)
    L = vrt.lib()
    cam, film = vrt.Camera(*pose_of(proxy_small, 6)), vrt.Film(1, 1, 72, 40)
    c, f = C.byref(cam.c), C.byref(film.c)
    vis = np.full((40, 72), 7.0, np.float32)
    p, d = vis.ctypes.data_as(_ffi.f32p), C.c_void_p(vis.ctypes.data)
    rays = C.c_int64(-7)
    inv = _ffi.VRT_E_INVALID
    for spp in (0, 65, -1):
        assert L.vrt_render_secondary_multi(m.h, c, f, spp, p, C.byref(rays)) == inv
        assert L.vrt_render_secondary_multi_device(m.h, c, f, spp, d, None) == inv
    assert L.vrt_render_secondary_multi(m.h, None, f, 64, p, None) == inv
    assert L.vrt_render_secondary_multi(m.h, c, None, 64, p, None) == inv
    assert L.vrt_render_secondary_multi(m.h, c, f, 64, None, C.byref(rays)) == inv
    assert L.vrt_render_secondary_multi_device(m.h, c, f, 64, None, None) == inv
    bad = vrt.Film(1, 1, 72, 40)
    bad.c.nx = 0
    with pytest.raises(vrt.VrtError) as e:
        m.render_secondary(cam, bad)
    assert e.value.status == inv
    assert rays.value == -7 and np.all(vis == 7.0)
    want, wrays = want_vis(proxy_small, 6, 72, 40, 64)
    got, r = m.render_secondary(cam, film, 64)  # the handle stays usable; rays may be NULL
    assert r == wrays and same_f32(got, want)
    assert L.vrt_render_secondary_multi(m.h, c, f, 64, p, None) == _ffi.VRT_OK and same_f32(vis, want)
