"""Cases for the cone march's fallback paths and the light pass's tail
hand-off (test_cone_paths_gpu.py, test_light_tail_gpu.py), and the conditions
that make them what they are meant to be, all from the oracle and the host
scene code alone (test_cone_paths_host.py asserts the same conditions without
a device).  A helper module: it holds no tests."""
import copy
import ctypes
import ctypes.util

import numpy as np

import pyoracle as po
import voxelraytrace20190722_amd as vrt

f32 = np.float32
LIGHT = (vrt.to_radian(60), (1.0, 10.0, 1.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))  # VRT/main.cc:80-83
VIEW = (vrt.to_radian(90), (1.0, 1.3, -0.2), (0.0, 0.4, 0.0), (0.0, 1.0, 0.0))  # VRT/main.cc:112-115
# the light camera turned away from the scene: every light sample misses
LIGHT_AWAY = (vrt.to_radian(60), (1.0, 10.0, 1.0), (1.0, 20.0, 1.0), (1.0, 0.0, 0.0))
FRAME = (40, 32)
KD_MAT = 9  # the proxy's untextured material (512 triangles)
KD_NONFINITE = (3e37, 1.0, 0.5)  # the light map's red sums overflow: lm_bad, cone_march_ref
KD_OVERFLOW = (1e38, 1e38, 1e38)  # a finite light map whose cone sums overflow
LIGHT_BUDGET = 768  # VRT_LIGHT_BUDGET: triangle tests before a light sample goes to the tail
CONE_STEPS = 1024  # kConeSteps: the step table's length
SCALE = f32(2.0 ** 20)  # case D: positions times a power of two (exact)
MV_DENORMAL = 1e-44  # case D: a denormal min_voxel (mindist = 10 units of 2^-149)
SWEEP_K = (-70, -40, -20, -8, -1, 0, 1, 6, 12)
SWEEP_J = (1, 4, 9)
# Case C's scene is the proxy with its positions times 149/128.  (int)log2f(x)
# and x's exponent e disagree for the floats from split_up[e] to just below
# 2^(e+1): one float for e + 1 = 3 and 4, none for 1 and 2, two to five for 5 to
# 12.  With the proxy's own diagonal (4.64349) no float diameter at all gives
# fl(maxdist / diam) = nextafter(16, 0) or nextafter(8, 0), so the table would
# decide only at levels that a depth-5 tree does not have; with this factor
# (the first of 1 + i/128 to do so) some min_voxel gives the first step each
# of 2, 16, 512 and their predecessors.
SWEEP_SCALE = f32(149.0 / 128.0)


_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.log2f.restype = ctypes.c_float
_libm.log2f.argtypes = [ctypes.c_float]


def log2f(x):
    """The C library's log2f, whose truncation is the reference's split level."""
    return f32(_libm.log2f(float(x)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_f32(a, b):
    """Bit-equal, NaN matching NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    return bool(np.all((np.isnan(a) & np.isnan(b)) | (bits(a) == bits(b))))


def classes(a):
    """0 finite, 1 +inf, 2 -inf, 3 NaN."""
    a = np.asarray(a, np.float32)
    return np.where(np.isnan(a), 3, np.where(a == np.inf, 1, np.where(a == -np.inf, 2, 0)))


def group_b(n=3000, scale=None):
    """The first n of the 3,000 "random interior rays" of
    test_trace_batch_gpu._groups (group b: rng seed 7, the first draws of
    that generator), restated; scale multiplies the origins."""
    rng = np.random.default_rng(7)
    o = (rng.uniform(-1, 1, (3000, 3)) * 0.8).astype(np.float32)
    o[:, 1] = np.abs(o[:, 1])
    d = rng.normal(0, 1, (3000, 3)).astype(np.float32)
    if scale is not None:
        o = (o * f32(scale)).astype(np.float32)
    return np.ascontiguousarray(np.stack([vrt.make_ray(o[i], d[i]) for i in range(n)]))


def with_kd(sd, kd):
    """sd with the untextured material's Kd replaced."""
    assert sd.mat_tex[KD_MAT] == -1 and (sd.mat == KD_MAT).sum() == 512
    out = copy.copy(sd)
    out.mat_kd = sd.mat_kd.copy()
    out.mat_kd[KD_MAT] = kd
    return out


def scaled(sd, scale):
    out = copy.copy(sd)
    out.pos = np.ascontiguousarray((sd.pos * f32(scale)).astype(np.float32))
    return out


def scaled_camera(cam, scale):
    fov, eye, spot, up = cam
    return (fov, tuple(float(f32(x) * f32(scale)) for x in eye), tuple(float(f32(x) * f32(scale)) for x in spot), up)


def light_rays(cam, nx, ny):
    """The light pass's rays: gen_rays4 of every pixel of the render area
    (the film cut to multiples of 8), in any order."""
    c, film = vrt.Camera(*cam), vrt.Film(1, 1, nx, ny)
    return np.concatenate([c.gen_rays4(film, px, py) for py in range(ny // 8 * 8) for px in range(nx // 8 * 8)])


def light_tests(osc, cam, nx, ny):
    """Per light sample, the triangle tests of the oracle's walk (an upper
    bound of the kernel's count, which skips leaves by their boxes), and hit."""
    m = osc.ray_march(light_rays(cam, nx, ny))
    return m["counters"][:, 2], m["hit"] == 1, m["tri"]


def oracle_lightmap(sd, depth, cam, nx, ny):
    osc = po.Scene(sd, depth)
    hits = osc.lightmap(po.camera(*cam), 1.0, 1.0, nx, ny, nthreads=8)
    return osc, hits


# ---- the float32 step sequence of k_cone_steps / cone_trace's loop header ----
def root_maxdist(box):
    """length(root.aabb.size()) as jql::length computes it: box (6,) float32."""
    size = (np.asarray(box[3:], np.float32) - np.asarray(box[:3], np.float32)).astype(np.float32)
    s = f32(0)
    for k in range(3):
        s = f32(s + f32(size[k] * size[k]))
    return np.sqrt(s)


_AP2 = f32(f32(0.577350269) * f32(2.0))


def first_diam(min_voxel):
    mind = f32(f32(1.414) * f32(min_voxel))
    d = f32(_AP2 * mind)
    return d if mind < d else mind


def cone_step_count(min_voxel, maxdist, cap=1 << 16):
    """Steps of the cone march's loop that pass both tests (dist < maxdist,
    not maxdist < diam), in float32 scalars."""
    mind = f32(f32(1.414) * f32(min_voxel))
    dist, n = mind, 0
    while dist < maxdist and n < cap:
        d = f32(_AP2 * dist)
        diam = d if mind < d else mind
        if maxdist < diam:
            break
        n += 1
        dist = f32(dist + f32(f32(0.1) * diam))
    return n


def _from_bits(b):
    return np.array(b, np.uint32).view(np.float32)[()]


def min_voxel_for_quotient(maxdist, target):
    """A float32 min_voxel whose first step has fl(maxdist / diam) == target
    exactly, by bisection over the bit patterns (the quotient does not grow
    with min_voxel) and a look at the neighbours; None if no float gives it."""
    target = f32(target)

    def q(b):
        with np.errstate(all="ignore"):
            return f32(f32(maxdist) / first_diam(_from_bits(b)))
    lo, hi = 1, 0x7F7FFFFF  # the least denormal .. FLT_MAX
    while lo < hi:  # the largest min_voxel with q >= target
        mid = lo + (hi - lo + 1) // 2
        if q(mid) >= target:
            lo = mid
        else:
            hi = mid - 1
    for b in sorted(range(max(lo - 64, 1), lo + 65), key=lambda b: abs(b - lo)):
        if q(b) == target:
            return _from_bits(b)
    return None


def sweep_scene(sd):
    """Case C's scene, light camera and rays (400 of group b), all times SWEEP_SCALE."""
    return scaled(sd, SWEEP_SCALE), scaled_camera(LIGHT, SWEEP_SCALE), group_b(400, SWEEP_SCALE)


def sweep_values(res, maxdist):
    """Case C's min_voxel values, ascending: res * 2^k, and per j the values
    that make the first quotient 2^j and its predecessor."""
    vals = [f32(f32(res) * f32(2.0 ** k)) for k in SWEEP_K]
    edge = {}
    for j in SWEEP_J:
        p2 = f32(2.0 ** j)
        edge[j] = (min_voxel_for_quotient(maxdist, p2), min_voxel_for_quotient(maxdist, np.nextafter(p2, f32(0))))
        vals += [v for v in edge[j] if v is not None]
    return sorted(set(float(v) for v in vals)), edge


def unlit_hit_triangles(osc, cam, nx, ny, rays, count):
    """The `count` triangles that the most of `rays` hit among those no light
    sample of the (nx, ny) light film hits."""
    _, lhit, ltri = light_tests(osc, cam, nx, ny)
    lit = np.unique(ltri[lhit])
    m = osc.ray_march(rays)
    tris, cnt = np.unique(m["tri"][m["hit"] == 1], return_counts=True)
    unlit = ~np.isin(tris, lit)
    order = np.argsort(-cnt[unlit], kind="stable")
    return tris[unlit][order][:count]


def zero_normals(sd, tris):
    out = copy.copy(sd)
    out.nrm = sd.nrm.copy()
    out.nrm[tris] = 0
    return out


def one_triangle():
    """A single slanted triangle under the light camera."""
    pos = np.array([[-3.0, 0.0, -3.0, 3.0, 1.5, -1.5, 0.0, 0.6, 3.0]], np.float32)
    e1, e2 = pos[0, 3:6] - pos[0, 0:3], pos[0, 6:9] - pos[0, 0:3]
    n = np.cross(e2, e1)
    n = (n / np.linalg.norm(n)).astype(np.float32)
    return vrt.SceneData(pos, np.tile(n, 3)[None, :])


# ---- restatements -------------------------------------------------------------
ILLUM_D = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1)], np.float32)


def _dot(a, b):
    s = np.zeros(np.broadcast(a[..., 0], b[..., 0]).shape, np.float32)
    for k in range(3):
        s = s + a[..., k] * b[..., k]
    return s


def compute_illum(L, d):
    """VoxelOctree::compute_illum (VRT/voxel_octree.h:72-82): L (m, 6, 3), d (m, 3)."""
    with np.errstate(all="ignore"):
        r = np.zeros((len(d), 3), np.float32)
        for i in range(6):
            s = _dot(ILLUM_D[i][None, :], d)
            coeff = np.where(s > f32(1), f32(1), np.where(s < f32(0), f32(0), s)).astype(np.float32)
            r = r + L[:, i, :] * coeff[:, None]
        return r


def direct_term(osc, depth, voxel, rays):
    """trace()'s direct term of hit rays: the hit leaf's compute_illum(-d) on
    the oracle's light map."""
    key, _, ill = osc.lightmap_nodes()
    leaf_key = (np.uint64(depth) << np.uint64(32)) | voxel.astype(np.uint64)
    at = np.searchsorted(key, leaf_key)
    assert np.array_equal(key[at], leaf_key)
    return compute_illum(ill[at], -rays[:, 3:6])
