"""Light probes on the GPU (vrt_probe_gather[_device]) against
LightProbe::gather_light (VRT/voxel_octree.cc:592-618) restated from the
oracle's ray_march and a float32 restatement of cone_trace (probe_cases.py),
which first proves itself on the probes' own rays against the batched trace()
the oracle pins.  Bar: bit-exact (NaN matching NaN)."""
import numpy as np
import pytest

import pyoracle as po
import voxelraytrace20190722_amd as vrt
from voxelraytrace20190722_amd import _ffi

import probe_cases as pc

pytestmark = pytest.mark.gpu

f32 = np.float32
VIEW = (vrt.to_radian(90), (1.0, 1.3, -0.2), (0.0, 0.4, 0.0), (0.0, 1.0, 0.0))  # VRT/main.cc:112-115
RADII = [0.1, 0, 0.05, 0.1, 0.3, 0.1, 0.1, 0.02, 0.1, 0.1, 1.0, 0.1]
LIGHT_COLOR = (0.7, 0.8, 0.9)


def _interior_probes(tree):
    mn, mx = tree.root_box
    c, ext = (mn + mx) / 2, (mx - mn) / 2
    rng = np.random.default_rng(11)
    o = (c + rng.uniform(-0.8, 0.8, (12, 3)) * ext).astype(f32)
    return np.ascontiguousarray(np.concatenate([o, np.array(RADII, f32)[:, None]], axis=1))


class Case:
    """One depth: the scene on both sides, the light map, the cone
    restatement, the twelve interior probes' expected values and the
    product's result for them, computed once."""

    def __init__(self, sd, depth):
        self.depth = depth
        self.tree = vrt.VoxelOctree(sd, depth)
        self.osc = po.Scene(sd, depth)
        hits = self.tree.lightmap(vrt.Camera(*pc.LIGHT), vrt.Film(1, 1, pc.LIGHT_N, pc.LIGHT_N))
        assert hits == self.osc.lightmap(po.camera(*pc.LIGHT), 1.0, 1.0, pc.LIGHT_N, pc.LIGHT_N, nthreads=8) > 0
        self.res = self.tree.min_voxel(6)
        assert self.res == self.osc.min_voxel(6)
        self.cone = pc.ConeTrace(self.tree)
        self.points = po.sphere_points(pc.SEED, 100)
        self.probes = _interior_probes(self.tree)
        self.want = pc.Expected(self.osc, self.cone, self.probes, self.points, self.res, LIGHT_COLOR)
        self.got, self.got_terms = self.tree.probe_gather(self.probes, self.res, LIGHT_COLOR, terms=True)
        for a in (self.probes, self.points, self.want.terms, self.want.a, self.want.hit, self.got_terms,
                  *self.got.values()):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def proxy_small():
    return vrt.SceneData.proxy(0.25, 2)


@pytest.fixture(scope="module")
def cases(proxy_small):
    made = {}

    def get(depth):
        if depth not in made:
            made[depth] = Case(proxy_small, depth)
        return made[depth]
    return get


def _check(got, terms, want, psel=slice(None), npts=None, what=""):
    """A gather's SGs (and terms, unless None) against the expected values of
    the probes want.*[psel], the first npts points of each group."""
    wt = want.terms[psel] if npts is None else want.terms[psel][:, :, :npts]
    if terms is not None:
        assert pc.same_f32(terms, wt), (what, "terms")
    assert pc.same_f32(got["a"], pc.seq_sum_div(wt)), (what, "a")
    assert np.array_equal(pc.bits(got["d"]), pc.bits(want.d[psel])), (what, "d")
    assert np.all(pc.bits(got["s"]) == pc.bits(f32(10))), (what, "s")


# ---- 1. twelve interior probes -------------------------------------------
@pytest.mark.parametrize("depth", [5, 7])
def test_interior_probes_match_expected(cases, depth):
    c = cases(depth)
    w = c.want
    # the restatement proves itself on the very rays of the bundle: the
    # batched trace()'s indirect term is the restated cone_trace, and that
    # call's rgb is the oracle's trace()
    rgb, parts = c.tree.trace(w.rays, c.res, parts=True)
    assert pc.same_f32(rgb, c.osc.shade_trace(w.rays, c.res))
    flat_hit = w.hit.reshape(-1)
    assert np.array_equal(parts["hit"] == 1, flat_hit)
    assert pc.same_f32(parts["hit_p"][flat_hit], w.hit_p[flat_hit])
    assert pc.same_f32(parts["normal"][flat_hit], w.normal[flat_hit])
    assert pc.same_f32(parts["indirect"][flat_hit], w.terms.reshape(-1, 3)[flat_hit])
    assert np.all(pc.bits(parts["indirect"][~flat_hit]) == 0)
    # the case is what it is meant to be (conditions on the oracle's values)
    share = flat_hit.mean()
    assert 0.6 <= share <= 0.95, share
    per_group = w.hit.reshape(-1, w.hit.shape[-1]).sum(axis=1)
    all_miss = per_group == 0
    mixed = (per_group > 0) & (per_group < w.hit.shape[-1])
    assert all_miss.sum() >= 3 and mixed.sum() >= 20, (all_miss.sum(), mixed.sum())
    ht = w.terms.reshape(-1, 3)[flat_hit]
    assert (np.all(np.isfinite(ht), axis=1) & np.any(ht != 0, axis=1)).mean() >= 0.5
    # the gather
    _check(c.got, c.got_terms, w, what=depth)
    assert np.array_equal(pc.bits(c.got["d"][0]), pc.bits(pc.normalize(pc.DIRS)))
    # an all-miss group's amplitude is the restated sum of light_color, which
    # is not light_color itself
    lc = np.array(LIGHT_COLOR, f32)
    miss_a = pc.seq_sum_div(np.tile(lc, (100, 1)))
    assert not np.array_equal(pc.bits(miss_a), pc.bits(lc))
    assert np.all(pc.bits(c.got["a"].reshape(-1, 3)[all_miss]) == pc.bits(miss_a))
    # without the terms
    assert pc.same_f32(c.tree.probe_gather(c.probes, c.res, LIGHT_COLOR)["a"], c.got["a"])


def test_lightprobe_class(cases):
    c = cases(5)
    lp = vrt.LightProbe(c.probes[4, :3], c.probes[4, 3])
    sgs = lp.gather_light(c.tree, c.res, LIGHT_COLOR)
    assert len(sgs) == 14
    assert pc.same_f32(np.stack([s.a for s in sgs]), c.want.a[4])
    dirs = pc.normalize(np.array([(0.3, 0.9, -0.2), (-1, 0, 0)], f32))
    want = pc.eval_restated(c.want.a[4:5], c.want.d[4:5], np.full((1, 14), 10, f32), dirs)[0]
    assert pc.same_f32(np.stack([lp.eval(d) for d in dirs]), want)


# ---- 2. edge probes ------------------------------------------------------------
def test_edge_probes(cases):
    c = cases(5)
    mn, mx = c.tree.root_box
    ctr, ext = (mn + mx) / 2, (mx - mn) / 2
    far = (ctr + np.array((5, 3, -4), f32) * ext).astype(f32)
    inside = c.probes[0, :3]
    nan_o = inside.copy()
    nan_o[1] = np.nan
    probes = np.array([(*far, 0.1), (*inside, 100 * float(np.abs(ext).max())), (*inside, 0.0), (*nan_o, 0.1),
                       (*c.probes[3, :3], 0.1)], f32)
    light = (np.inf, -0.0, 0.7)
    want = pc.Expected(c.osc, c.cone, probes, c.points, c.res, light)
    assert not want.hit[1].any()  # tmin lies beyond the scene
    assert want.hit[2].any() and want.hit[4].any()
    got, terms = c.tree.probe_gather(probes, c.res, light, terms=True)
    _check(got, terms, want, what="edge")
    # an all-miss group: inf, the sum of -0.0 from +0 is +0, and 0.7's sum
    assert np.isposinf(got["a"][1, 0, 0]) and pc.bits(got["a"][1, 0, 1]) == 0
    assert np.all(pc.bits(terms[1, :, :, 1]) == 0x80000000)


# ---- 3. sizes ------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_probe_counts(cases, n):
    c = cases(5)
    got, terms = c.tree.probe_gather(c.probes[:n], c.res, LIGHT_COLOR, terms=True)
    assert got["a"].shape == (n, 14, 3) and terms.shape == (n, 14, 100, 3)
    _check(got, terms, c.want, slice(0, n), what=n)


@pytest.fixture(scope="module")
def custom(cases):
    """Three probes with 129 points of the caller's: a prefix of the points
    gives the same rays, so one expected set serves every npoints."""
    c = cases(5)
    points = po.sphere_points(0x5eed, 129)
    probes = np.ascontiguousarray(c.probes[[4, 1, 7]])
    return c, probes, points, pc.Expected(c.osc, c.cone, probes, points, c.res, LIGHT_COLOR)


@pytest.mark.parametrize("npts", [1, 63, 64, 65, 100, 129])
def test_caller_points(custom, npts):
    c, probes, points, want = custom
    assert want.hit.any() and not want.hit.all()
    got, terms = c.tree.probe_gather(probes, c.res, LIGHT_COLOR, points=points[:npts], terms=True)
    assert terms.shape == (3, 14, npts, 3)
    _check(got, terms, want, npts=npts, what=npts)


def test_default_points_are_probe_points(cases):
    c = cases(5)
    assert np.array_equal(pc.bits(vrt.probe_points()), pc.bits(c.points))
    got, terms = c.tree.probe_gather(c.probes[:3], c.res, LIGHT_COLOR, points=vrt.probe_points(), terms=True)
    assert pc.same_f32(got["a"], c.got["a"][:3]) and pc.same_f32(terms, c.got_terms[:3])
    with pytest.raises(vrt.VrtError) as e:
        c.tree.probe_gather(c.probes[:1], c.res, LIGHT_COLOR, points=np.zeros((1025, 3), f32))
    assert e.value.status == _ffi.VRT_E_INVALID
    with pytest.raises(vrt.VrtError) as e:
        c.tree.probe_gather(c.probes[:1], c.res, LIGHT_COLOR, points=np.zeros((0, 3), f32))
    assert e.value.status == _ffi.VRT_E_INVALID
    # min_voxel <= 0 is the scene's Res
    assert pc.same_f32(c.tree.probe_gather(c.probes[:2], 0.0, LIGHT_COLOR)["a"],
                       c.tree.probe_gather(c.probes[:2], c.tree.min_voxel(0), LIGHT_COLOR)["a"])


# ---- 4. chunk seams ------------------------------------------------------------
def test_chunk_seams(cases):
    c = cases(5)
    vrt.set_test_flags(vrt.TEST_SMALL_PROBE_CHUNK)
    try:
        got, terms = c.tree.probe_gather(c.probes[:5], c.res, LIGHT_COLOR, terms=True)
    finally:
        vrt.set_test_flags(0)
    _check(got, terms, c.want, slice(0, 5), what="2-probe chunks")
    for key in got:
        assert pc.same_f32(got[key], c.got[key][:5]), key
    assert pc.same_f32(terms, c.got_terms[:5])


# ---- 5. the device variant -------------------------------------------------------
SENTINEL = 12345.0


def test_device_variant_equals_host_variant(cases, proxy_small):
    import torch
    c = cases(5)
    n = len(c.probes)
    d_probes = torch.from_numpy(c.probes.copy()).cuda()
    tail = 1024
    st = torch.cuda.Stream()
    for flags in (0, vrt.TEST_SMALL_PROBE_CHUNK):
        for with_terms in (True, False):
            d_sgs = torch.full((n * 14 * 7 + tail,), SENTINEL, device="cuda")
            d_terms = torch.full((n * 14 * 100 * 3 + tail,), SENTINEL, device="cuda")
            torch.cuda.synchronize()
            vrt.set_test_flags(flags)
            try:
                c.tree.probe_gather_device(d_probes.data_ptr(), n, d_sgs.data_ptr(), c.res, LIGHT_COLOR,
                                           d_terms_ptr=d_terms.data_ptr() if with_terms else None,
                                           stream_ptr=st.cuda_stream)
            finally:
                vrt.set_test_flags(0)
            st.synchronize()
            sgs, terms = d_sgs.cpu().numpy(), d_terms.cpu().numpy()
            assert np.all(sgs[n * 14 * 7:] == SENTINEL) and np.all(terms[n * 14 * 100 * 3:] == SENTINEL)
            rec = sgs[:n * 14 * 7].reshape(n, 14, 7)
            assert pc.same_f32(rec[:, :, 0:3], c.got["a"]), (flags, with_terms)
            assert pc.same_f32(rec[:, :, 3:6], c.got["d"]) and pc.same_f32(rec[:, :, 6], c.got["s"])
            if with_terms:
                assert pc.same_f32(terms[:n * 14 * 100 * 3].reshape(n, 14, 100, 3), c.got_terms), flags
            else:
                assert np.all(terms == SENTINEL)
    # caller's points, the null stream
    pts = po.sphere_points(3, 65)
    d_sgs = torch.full((2 * 14 * 7 + tail,), SENTINEL, device="cuda")
    torch.cuda.synchronize()
    c.tree.probe_gather_device(d_probes.data_ptr(), 2, d_sgs.data_ptr(), c.res, LIGHT_COLOR, points=pts)
    torch.cuda.synchronize()
    sgs = d_sgs.cpu().numpy()
    assert np.all(sgs[2 * 14 * 7:] == SENTINEL)
    assert pc.same_f32(sgs[:2 * 14 * 7].reshape(2, 14, 7)[:, :, 0:3],
                       c.tree.probe_gather(c.probes[:2], c.res, LIGHT_COLOR, points=pts)["a"])
    # errors that need a device: no light map yet, NULL required pointers
    fresh = vrt.VoxelOctree(proxy_small, 3)
    for call in (lambda: fresh.probe_gather(c.probes[:2], 0.0, LIGHT_COLOR),
                 lambda: fresh.probe_gather_device(d_probes.data_ptr(), 2, d_sgs.data_ptr())):
        with pytest.raises(vrt.VrtError) as e:
            call()
        assert e.value.status == _ffi.VRT_E_INVALID and "no light map" in str(e.value)
    L = vrt.lib()
    lc = np.array(LIGHT_COLOR, f32)
    lp = _ffi.ptr(lc, _ffi.f32p)
    assert L.vrt_probe_gather_device(c.tree.h, None, 2, 0.0, lp, None, 0, d_sgs.data_ptr(), None,
                                     None) == _ffi.VRT_E_INVALID
    assert L.vrt_probe_gather_device(c.tree.h, d_probes.data_ptr(), 2, 0.0, None, None, 0, d_sgs.data_ptr(), None,
                                     None) == _ffi.VRT_E_INVALID
    assert L.vrt_probe_gather_device(c.tree.h, d_probes.data_ptr(), 2, 0.0, lp, None, 0, None, None,
                                     None) == _ffi.VRT_E_INVALID
    assert L.vrt_probe_gather_device(c.tree.h, d_probes.data_ptr(), -1, 0.0, lp, None, 0, d_sgs.data_ptr(), None,
                                     None) == _ffi.VRT_E_INVALID
    assert L.vrt_probe_gather_device(c.tree.h, None, 0, 0.0, None, None, 0, None, None, None) == _ffi.VRT_OK
    torch.cuda.synchronize()
    assert np.all(d_sgs.cpu().numpy()[2 * 14 * 7:] == SENTINEL)


def test_scratch_does_not_grow_with_probe_count(cases, proxy_small):
    c = cases(5)
    tree = vrt.VoxelOctree(proxy_small, 4)
    tree.lightmap(vrt.Camera(*pc.LIGHT), vrt.Film(1, 1, 64, 64))
    before = tree.scratch_bytes()[0]
    vrt.set_test_flags(vrt.TEST_SMALL_PROBE_CHUNK)
    try:
        tree.probe_gather(c.probes[:2], 0.0, LIGHT_COLOR, terms=True)
        b2 = tree.scratch_bytes()[0]
        tree.probe_gather(c.probes[:7], 0.0, LIGHT_COLOR, terms=True)
        b7 = tree.scratch_bytes()[0]
    finally:
        vrt.set_test_flags(0)
    # one chunk of 2 probes: 64-B records (+ 4 B) per ray and the staging of
    # the probes, SGs and terms; nothing that grows with n
    rays = 2 * 14 * 100
    assert before < b2 == b7 <= before + rays * 68 + 1024 * 16 + 1024 + 2 * (16 + 14 * 28) + rays * 12


def test_gather_between_frames_on_streams(proxy_small):
    """A gather on a side stream between two one-call frames on another
    stream, the frames with different light passes: the gather reads the
    first frame's light map (the current one when it is enqueued)."""
    import torch
    tree, osc = vrt.VoxelOctree(proxy_small, 5), po.Scene(proxy_small, 5)
    lfilm = vrt.Film(1, 1, 96, 96)
    film = vrt.Film(1, 1, 40, 32)
    tree.lightmap(vrt.Camera(*pc.LIGHT), lfilm)
    osc.lightmap(po.camera(*pc.LIGHT), 1.0, 1.0, 96, 96, nthreads=8)
    res = tree.min_voxel(6)
    probes = _interior_probes(tree)[[4, 2]]
    points = po.sphere_points(pc.SEED, 100)
    want = pc.Expected(osc, pc.ConeTrace(tree), probes, points, res, LIGHT_COLOR)
    want1 = osc.render_trace(po.camera(*VIEW), 1.0, 1.0, 40, 32, res, samples=False)
    light2 = (vrt.to_radian(45), (-2.0, 8.0, 3.0), (0.0, 0.5, 0.0), (0.0, 1.0, 0.0))
    osc.lightmap(po.camera(*light2), 1.0, 1.0, 96, 96, nthreads=8)
    want2 = osc.render_trace(po.camera(*VIEW), 1.0, 1.0, 40, 32, res, samples=False)
    assert not np.array_equal(pc.bits(want1), pc.bits(want2))
    main, side = torch.cuda.Stream(), torch.cuda.Stream()
    img1, img2 = (torch.zeros((32, 40, 3), device="cuda") for _ in range(2))
    d_probes = torch.from_numpy(probes.copy()).cuda()
    d_sgs = torch.zeros((2, 14, 7), device="cuda")
    d_terms = torch.zeros((2, 14, 100, 3), device="cuda")
    torch.cuda.synchronize()
    tree.trace_frame_device(vrt.Camera(*pc.LIGHT), lfilm, vrt.Camera(*VIEW), film, 0, 1, 1, img1.data_ptr(), res,
                            main.cuda_stream)
    tree.probe_gather_device(d_probes.data_ptr(), 2, d_sgs.data_ptr(), res, LIGHT_COLOR,
                             d_terms_ptr=d_terms.data_ptr(), stream_ptr=side.cuda_stream)
    tree.trace_frame_device(vrt.Camera(*light2), lfilm, vrt.Camera(*VIEW), film, 0, 1, 1, img2.data_ptr(), res,
                            main.cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(pc.bits(img1.cpu().numpy()), pc.bits(want1))
    assert np.array_equal(pc.bits(img2.cpu().numpy()), pc.bits(want2))
    assert pc.same_f32(d_terms.cpu().numpy(), want.terms)
    assert pc.same_f32(d_sgs.cpu().numpy()[:, :, 0:3], want.a)
    # and the light map is now the second one: a new gather differs
    assert not pc.same_f32(tree.probe_gather(probes, res, LIGHT_COLOR)["a"], want.a)
