"""The cone march's three bodies (cone_march in csrc/vrt_kernels.hip) through
the three kernels that share them (k_cones_film: render_trace, k_cones_batch:
vrt_trace_batch / vrt_cone_trace_batch, k_probe_cones: vrt_probe_gather),
against the oracle's trace():

  A  a light map with +inf entries      -> cone_march_ref (lm_bad)
  B  a finite light map, sums overflow  -> cone_march_axes
  C  a min_voxel sweep                  -> the step table and split_level_of
  D  more than 1,024 steps              -> cone_march_fast for every cone
  E  a NaN cone direction               -> cone_march_fast for that cone

The cases and the conditions that make them what they are meant to be are in
cone_path_cases.py (test_cone_paths_host.py asserts the conditions without a
device).  Bar: bit-exact; where the oracle's value is NaN, a NaN."""
import numpy as np
import pytest

import pyoracle as po
import voxelraytrace20190722_amd as vrt

import cone_path_cases as cc
import probe_cases as pc

pytestmark = pytest.mark.gpu

f32 = np.float32
LIGHT_COLOR = (0.7, 0.8, 0.9)


def _check_classes(got, want, what):
    """Per channel the same class (finite / +inf / -inf / NaN), and the same
    bits wherever the oracle's value is not NaN."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, what
    assert np.array_equal(cc.classes(got), cc.classes(want)), what
    ok = ~np.isnan(want)
    assert np.array_equal(cc.bits(got)[ok], cc.bits(want)[ok]), what


class Case:
    """A scene on both sides with its light map, the rays' oracle values and
    the product's whole-batch result, computed once."""

    def __init__(self, sd, depth, light, light_n, rays, min_voxel=None):
        self.depth = depth
        self.tree = vrt.VoxelOctree(sd, depth)
        self.osc = po.Scene(sd, depth)
        hits = self.tree.lightmap(vrt.Camera(*light), vrt.Film(1, 1, light_n, light_n))
        assert hits == self.osc.lightmap(po.camera(*light), 1.0, 1.0, light_n, light_n, nthreads=8) > 0
        self.res = self.tree.min_voxel(6) if min_voxel is None else min_voxel
        assert min_voxel is not None or self.res == self.osc.min_voxel(6)
        self.rays = rays
        self.want_rgb = self.osc.shade_trace(rays, self.res)
        self.want_hit = self.osc.ray_march(rays)
        self.hit = self.want_hit["hit"] == 1
        self.rgb, self.parts = self.tree.trace(rays, self.res, parts=True)
        for a in (self.want_rgb, self.rgb, *self.want_hit.values(), *self.parts.values()):
            a.setflags(write=False)

    def check_march(self):
        for key in ("hit", "tri", "voxel"):
            assert np.array_equal(self.parts[key], self.want_hit[key]), key
        for key in ("hit_p", "normal"):
            assert cc.same_f32(self.parts[key], self.want_hit[key]), key

    def lightmap_equal(self):
        for got, want in zip(self.tree.lightmap_nodes(), self.osc.lightmap_nodes()):
            if got.dtype == np.float32:
                assert cc.same_f32(got, want)
                assert np.array_equal(np.isfinite(got), np.isfinite(want))
            else:
                assert np.array_equal(got, want)
        return self.tree.lightmap_nodes()


@pytest.fixture(scope="module")
def proxy_small():
    return vrt.SceneData.proxy(0.25, 2)


@pytest.fixture(scope="module")
def rays_b():
    rays = cc.group_b()
    rays.setflags(write=False)
    return rays


@pytest.fixture(scope="module")
def plain(proxy_small, rays_b):
    """The proxy as it is (depth 5, light film 64 x 64)."""
    return Case(proxy_small, 5, cc.LIGHT, 64, rays_b)


@pytest.fixture(scope="module")
def case_a(proxy_small, rays_b):
    return Case(cc.with_kd(proxy_small, cc.KD_NONFINITE), 5, cc.LIGHT, 256, rays_b)


@pytest.fixture(scope="module")
def case_b(proxy_small, rays_b):
    return Case(cc.with_kd(proxy_small, cc.KD_OVERFLOW), 5, cc.LIGHT, 128, rays_b)


# ---- A. a light map that is not finite: cone_march_ref ------------------------
def test_nonfinite_lightmap_equals_oracle(case_a):
    _, cov, ill = case_a.lightmap_equal()
    assert np.isfinite(cov).all()
    assert (~np.isfinite(ill)).sum() >= 1 and not np.isnan(ill).any()  # +inf entries: lm_bad is raised


def test_nonfinite_lightmap_batch(case_a, plain, proxy_small):
    c = case_a
    # the case is what it is meant to be (the oracle's values)
    cls = cc.classes(c.want_rgb[c.hit])
    assert ((cls[:, 0] == 1) & ~(cls == 3).any(axis=1)).sum() >= 100
    assert (cls[:, 0] == 3).sum() >= 1000
    gb = c.want_rgb[c.hit][:, 1:]
    assert (np.isfinite(gb).all(axis=1) & (gb != 0).all(axis=1)).mean() >= 0.9
    # the batch
    c.check_march()
    _check_classes(c.rgb, c.want_rgb, "rgb")
    hi = np.flatnonzero(c.hit)
    # direct: the hit leaf's compute_illum(-d) on the oracle's light map
    assert cc.same_f32(c.parts["direct"][hi], cc.direct_term(c.osc, c.depth, c.parts["voxel"][hi], c.rays[hi]))
    # albedo: the changed Kd on its material's triangles, elsewhere what the
    # proxy as it is gives (its rgb is pinned below)
    changed = proxy_small.mat[c.parts["tri"][hi]] == cc.KD_MAT
    assert 0 < changed.sum() < len(hi)
    assert np.all(cc.bits(c.parts["albedo"][hi][changed]) == cc.bits(np.array(cc.KD_NONFINITE, f32)))
    assert np.array_equal(cc.bits(c.parts["albedo"][hi][~changed]), cc.bits(plain.parts["albedo"][hi][~changed]))
    assert cc.same_f32(plain.rgb, plain.want_rgb)
    for key in ("indirect", "direct", "albedo"):
        assert np.all(cc.bits(c.parts[key][~c.hit]) == 0), key
    # rgb = albedo * (indirect + direct) where all three are finite
    ind, dr, alb = (c.parts[k][hi] for k in ("indirect", "direct", "albedo"))
    fin = np.isfinite(ind) & np.isfinite(dr) & np.isfinite(alb)
    with np.errstate(all="ignore"):
        assert np.array_equal(cc.bits(alb * (ind + dr))[fin], cc.bits(c.rgb[hi])[fin])


def test_nonfinite_lightmap_frame(case_a):
    """k_cones_film on the same light map."""
    c = case_a
    nx, ny = cc.FRAME
    got = c.tree.render_trace(vrt.Camera(*cc.VIEW), vrt.Film(1, 1, nx, ny), c.res)
    want = c.osc.render_trace(po.camera(*cc.VIEW), 1.0, 1.0, nx, ny, c.res, samples=False)
    assert np.isnan(want).sum() >= 100 and np.isfinite(want).sum() >= 100
    _check_classes(got, want, "frame")


def test_nonfinite_lightmap_cone_batch(case_a):
    """k_cones_batch on the batch's own hit points and normals."""
    c = case_a
    hi = np.flatnonzero(c.hit)
    out = c.tree.cone_trace(c.parts["hit_p"][hi], c.parts["normal"][hi], c.res)
    _check_classes(out, c.parts["indirect"][hi], "cone batch")


def test_nonfinite_lightmap_probe_gather(case_a):
    """k_probe_cones on the same light map: three probes against the restated
    gather, whose cone restatement first reproduces the batch's indirect
    term (which the oracle pins through rgb)."""
    c = case_a
    cone = pc.ConeTrace(c.tree)
    hi = np.flatnonzero(c.hit)[:64]
    _check_classes(c.parts["indirect"][hi], cone(c.parts["hit_p"][hi], c.parts["normal"][hi], c.res), "restatement")
    mn, mx = c.tree.root_box
    ctr, ext = (mn + mx) / 2, (mx - mn) / 2
    o = (ctr + np.random.default_rng(11).uniform(-0.8, 0.8, (3, 3)) * ext).astype(f32)
    probes = np.ascontiguousarray(np.concatenate([o, np.full((3, 1), 0.1, f32)], axis=1))
    points = po.sphere_points(pc.SEED, 100)
    want = pc.Expected(c.osc, cone, probes, points, c.res, LIGHT_COLOR)
    ht = want.terms[want.hit]
    assert len(ht) >= 1000 and np.isnan(ht).any() and np.isfinite(ht).any()
    got, terms = c.tree.probe_gather(probes, c.res, LIGHT_COLOR, terms=True)
    assert pc.same_f32(terms, want.terms)
    assert np.array_equal(np.isfinite(terms), np.isfinite(want.terms))
    assert pc.same_f32(got["a"], pc.seq_sum_div(want.terms))
    assert np.array_equal(pc.bits(got["d"]), pc.bits(want.d))
    assert np.all(pc.bits(got["s"]) == pc.bits(f32(10)))


# ---- B. overflow on the production path -----------------------------------------
def test_overflow_on_finite_lightmap(case_b):
    c = case_b
    _, cov, ill = c.lightmap_equal()
    assert np.isfinite(ill).all() and np.isfinite(cov).all()  # lm_bad stays 0: cone_march_axes
    cls = cc.classes(c.want_rgb[c.hit])
    assert (cls == 1).any(axis=1).sum() >= 20 and not (cls == 3).any()
    c.check_march()
    assert np.array_equal(cc.bits(c.rgb), cc.bits(c.want_rgb))
    nx, ny = cc.FRAME
    got = c.tree.render_trace(vrt.Camera(*cc.VIEW), vrt.Film(1, 1, nx, ny), c.res)
    want = c.osc.render_trace(po.camera(*cc.VIEW), 1.0, 1.0, nx, ny, c.res, samples=False)
    assert (want == np.inf).any() and not np.isnan(want).any()
    assert np.array_equal(cc.bits(got), cc.bits(want))


# ---- C. a min_voxel sweep -------------------------------------------------------
def test_min_voxel_sweep(proxy_small):
    """res * 2^k down to split levels past 63 and up to a march of no step,
    and the values whose first step divides to 2^j and to the float below it,
    where (int)log2f and the exponent disagree and split_up decides (j = 4:
    levels 4 and 3, both in this tree)."""
    sd, light, rays = cc.sweep_scene(proxy_small)
    c = Case(sd, 5, light, 64, rays)
    _, cov, ill = c.lightmap_equal()
    assert np.isfinite(ill).all()
    maxdist = cc.root_maxdist(np.concatenate(c.tree.root_box))
    assert maxdist == cc.root_maxdist(c.osc.info()[1])
    vals, edge = cc.sweep_values(c.res, maxdist)
    assert len(vals) == len(cc.SWEEP_K) + 2 * len(cc.SWEEP_J) and all(v is not None for j in edge for v in edge[j])
    assert c.hit.sum() >= 300
    want = {v: c.osc.shade_trace(rays, v) for v in vals}
    for a, b in zip(vals, vals[1:]):
        twins = any(set(edge[j]) == {f32(a), f32(b)} for j in cc.SWEEP_J)
        differ = np.any(cc.bits(want[a][c.hit]) != cc.bits(want[b][c.hit]), axis=1).mean()
        assert twins or differ >= 0.5, (a, b, differ)
    for v in vals:
        assert np.array_equal(cc.bits(c.tree.trace(rays, v)), cc.bits(want[v])), v
    # the step table's rebuild key: to another value and back, on one trace
    # set, from both ends and about each power of two
    at4, below4 = (float(v) for v in edge[4])
    for seq in ([vals[0], vals[-1], vals[0]], [vals[-1], vals[0], vals[-1]], [at4, below4, at4, below4],
                [float(edge[1][1]), float(edge[9][0]), float(edge[1][1])], [c.res, vals[0], c.res]):
        for v in seq:
            assert np.array_equal(cc.bits(c.tree.trace(rays, v)), cc.bits(want[v])), (seq, v)
    # and through a frame (k_cones_film) at the two values about 16
    nx, ny = cc.FRAME
    view = cc.scaled_camera(cc.VIEW, cc.SWEEP_SCALE)
    for v in (below4, at4, vals[0]):
        got = c.tree.render_trace(vrt.Camera(*view), vrt.Film(1, 1, nx, ny), v)
        assert np.array_equal(cc.bits(got), cc.bits(c.osc.render_trace(po.camera(*view), 1.0, 1.0, nx, ny, v,
                                                                        samples=False))), v


# ---- D. more steps than the table holds ---------------------------------------------
def test_more_steps_than_the_table(proxy_small):
    """A denormal min_voxel on the proxy scaled by 2^20: the float32 step
    count passes kConeSteps, k_cone_steps reports -1 and every cone takes
    cone_march_fast.  (The oracle: 64 rays in 0.03 s, the frame in under a
    second.)"""
    sd = cc.scaled(proxy_small, cc.SCALE)
    rays = cc.group_b(64, cc.SCALE)
    c = Case(sd, 5, cc.scaled_camera(cc.LIGHT, cc.SCALE), 64, rays, min_voxel=cc.MV_DENORMAL)
    _, cov, ill = c.lightmap_equal()
    assert np.isfinite(ill).all()
    maxdist = cc.root_maxdist(np.concatenate(c.tree.root_box))
    assert cc.cone_step_count(cc.MV_DENORMAL, maxdist) > cc.CONE_STEPS
    assert c.hit.sum() >= 50 and np.isfinite(c.want_rgb).all() and np.any(c.want_rgb[c.hit] != 0, axis=1).all()
    c.check_march()
    assert np.array_equal(cc.bits(c.rgb), cc.bits(c.want_rgb))
    hi = np.flatnonzero(c.hit)
    out = c.tree.cone_trace(c.parts["hit_p"][hi], c.parts["normal"][hi], cc.MV_DENORMAL)
    assert np.array_equal(cc.bits(out), cc.bits(c.parts["indirect"][hi]))
    view = cc.scaled_camera(cc.VIEW, cc.SCALE)
    got = c.tree.render_trace(vrt.Camera(*view), vrt.Film(1, 1, 24, 16), cc.MV_DENORMAL)
    want = c.osc.render_trace(po.camera(*view), 1.0, 1.0, 24, 16, cc.MV_DENORMAL, samples=False)
    assert np.array_equal(cc.bits(got), cc.bits(want))
    # back within the table on the same trace set
    res = c.tree.min_voxel(6)
    assert cc.cone_step_count(res, maxdist) <= cc.CONE_STEPS
    assert np.array_equal(cc.bits(c.tree.trace(rays, res)), cc.bits(c.osc.shade_trace(rays, res)))
    assert np.array_equal(cc.bits(c.tree.trace(rays, cc.MV_DENORMAL)), cc.bits(c.want_rgb))


# ---- E. a NaN cone direction on a finite light map ---------------------------------
def test_nan_cone_direction(plain, proxy_small, rays_b):
    """Zero normals on five triangles that no light sample hits and group-b
    rays do: their hits' cones have NaN directions (cone_march's "twin"
    branch) while the light map stays finite."""
    tris = cc.unlit_hit_triangles(plain.osc, cc.LIGHT, 64, 64, rays_b, 5)
    c = Case(cc.zero_normals(proxy_small, tris), 5, cc.LIGHT, 64, rays_b)
    _, cov, ill = c.lightmap_equal()
    assert np.isfinite(ill).all()
    for got, was in zip(c.tree.lightmap_nodes(), plain.tree.lightmap_nodes()):
        assert np.array_equal(cc.bits(got), cc.bits(was))  # (uint64 keys as pairs of words)
    on = c.hit & np.isin(c.want_hit["tri"], tris)
    assert on.sum() >= 50 and np.isnan(c.want_rgb[on]).all() and np.isfinite(c.want_rgb[~on]).all()
    c.check_march()
    assert cc.same_f32(c.rgb, c.want_rgb)
    assert np.isnan(c.parts["indirect"][on]).all()
    assert np.isfinite(c.parts["direct"][on]).all()
    assert np.array_equal(cc.bits(c.parts["direct"][on]), cc.bits(plain.parts["direct"][on]))
    assert cc.same_f32(c.parts["direct"][on], cc.direct_term(c.osc, 5, c.parts["voxel"][on], rays_b[on]))
    # every other ray as in the scene without the edit
    assert cc.same_f32(plain.rgb, plain.want_rgb)
    assert np.array_equal(cc.bits(c.rgb[~on]), cc.bits(plain.rgb[~on]))
    for key in c.parts:  # (all 4-byte types)
        assert np.array_equal(cc.bits(c.parts[key][~on]), cc.bits(plain.parts[key][~on])), key
