"""Cases shared by tests/test_reference_gi_host.py, tests/test_reference_gi_gpu.py
and the ref_gi section of tests/golden/make_golden.py: the scenes, cameras,
films, ray batches, lights and probes on which the oracle and the HIP paths are
compared with the reference's own compiled camera.cc / voxel_octree.cc
(oracle/_ref/libvrtref_gi.so behind oracle/ref_gi_glue.cc), and the float32
combine of trace() the reference keeps in main.cc.  A helper module: it holds
no tests and touches no GPU."""
import ctypes
import ctypes.util
import os

import numpy as np

import pyoracle as po
import voxelraytrace20190722_amd as vrt

F = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
UP = (0.0, 1.0, 0.0)
LIGHT = (vrt.to_radian(60), (1.0, 10.0, 1.0), (0.0, 0.0, 0.0), UP)  # VRT/main.cc:76-78
VIEW = (vrt.to_radian(90), (1.0, 1.3, -0.2), (0.0, 0.4, 0.0), UP)   # VRT/main.cc:112-115
LIGHT2 = (vrt.to_radian(75), (-4.0, 6.0, 2.5), (0.5, 0.5, 0.0), UP)
COLOR2 = (0.25, 1.5, 0.7)
PROBE_LIGHT = (0.7, 0.8, 0.9)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_f32(a, b):
    """Bit-equal, NaN matching NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    return bool(np.all((np.isnan(a) & np.isnan(b)) | (bits(a) == bits(b))))


def diff_count(a, b):
    """Elements (rows, for 2-D input) that differ in bits, NaN matching NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ne = ~((np.isnan(a) & np.isnan(b)) | (bits(a) == bits(b)))
    return int(ne.reshape(len(a), -1).any(axis=1).sum()) if a.ndim else int(ne)


# ---- scenes -----------------------------------------------------------------------
def downsample_textures(sd, step):
    dims, offs, data = [], [], []
    o = 0
    for t in range(len(sd.tex_off)):
        w, h, c = sd.tex_dims[t]
        img = sd.tex_data[sd.tex_off[t]: sd.tex_off[t] + w * h * c].reshape(h, w, c)[::step, ::step]
        img = np.ascontiguousarray(img)
        dims.append([img.shape[1], img.shape[0], c])
        offs.append(o)
        data.append(img.reshape(-1))
        o += img.size
    return vrt.SceneData(sd.pos, sd.nrm, sd.uv, sd.mat, sd.mat_tex, sd.mat_kd, np.array(dims, np.int32),
                         np.array(offs, np.int64), np.concatenate(data))


def proxy_scene():
    """The proxy of the scene_proxy fixture: 1-, 3- and 4-channel textures
    and an untextured material."""
    return downsample_textures(vrt.SceneData.proxy(0.02, 1), 8)


def scene_from(z, prefix=""):
    g = lambda k: z[prefix + k]
    return vrt.SceneData(g("pos"), g("nrm"), g("uv"), g("mat"), g("mat_tex"), g("mat_kd"), g("tex_dims"),
                         g("tex_off"), g("tex_data"))


def scene_arrays(sd, prefix=""):
    return {prefix + k: getattr(sd, k) for k in ("pos", "nrm", "uv", "mat", "mat_tex", "mat_kd", "tex_dims",
                                                  "tex_off", "tex_data")}


def write_tga(path, img):
    """An uncompressed top-left-origin TGA that stbi_load decodes to exactly
    img (h, w, c) uint8, c in 1 (grey), 3, 4."""
    h, w, c = img.shape
    assert c in (1, 3, 4)
    hdr = bytearray(18)
    hdr[2] = 3 if c == 1 else 2
    hdr[12:14] = int(w).to_bytes(2, "little")
    hdr[14:16] = int(h).to_bytes(2, "little")
    hdr[16] = 8 * c
    hdr[17] = 0x20 | (8 if c == 4 else 0)
    px = img if c == 1 else img[:, :, [2, 1, 0] + ([3] if c == 4 else [])]
    with open(path, "wb") as f:
        f.write(bytes(hdr))
        f.write(np.ascontiguousarray(px).tobytes())


def texture_files(sd, dirpath, tag):
    """The scene's textures as files for the reference's texel_fetch: one name
    per material (None: untextured).  The reference caches textures by name
    for the life of the process, so tag must be unique per scene."""
    names = []
    for m, t in enumerate(np.asarray(sd.mat_tex)):
        if t < 0:
            names.append(None)
            continue
        w, h, c = (int(v) for v in sd.tex_dims[t])
        off = int(sd.tex_off[t])
        path = os.path.join(str(dirpath), f"{tag}_tex{int(t)}.tga")
        if not os.path.exists(path):
            write_tga(path, np.asarray(sd.tex_data[off:off + w * h * c]).reshape(h, w, c))
        names.append(path)
    return names


def single_triangle():
    return vrt.SceneData(np.array([[-5, -5, -1, 5, -5, -1, 0, 5, -1]], F), np.ones((1, 9), F))


# ---- cameras and films --------------------------------------------------------------
def cameras(mn, mx):
    """main()'s two cameras, two sweep poses, and three awkward ones: straight
    down an axis, `up` nearly parallel to the view, a 0.05 degree fov."""
    c = (np.asarray(mn, np.float64) + mx) / 2
    sweep = [(f, tuple(float(v) for v in e), tuple(float(v) for v in s), tuple(float(v) for v in u))
             for f, e, s, u in (vrt.sweep_pose(mn, mx, i, 16) for i in (3, 11))]
    return {
        "light": LIGHT, "view": VIEW, "sweep3": sweep[0], "sweep11": sweep[1],
        "axis": (vrt.to_radian(60), (float(c[0]), float(c[1]), float(mx[2]) + 2.0),
                 (float(c[0]), float(c[1]), float(c[2])), UP),
        "up_parallel": (vrt.to_radian(70), (0.3, float(mx[1]) + 3.0, 0.2), (0.3, float(c[1]), 0.2001), UP),
        "narrow": (vrt.to_radian(0.05), VIEW[1], VIEW[2], UP),
    }


FILMS = ((1.0, 1.0, 16, 16), (1.5, 0.75, 24, 8))


def oracle_film_rays(cam, film_w, film_h, nx, ny, four=True, near=0.0, far=FLT_MAX):
    """The oracle's gen_rays4 / gen_rays1 on every pixel -> (ny, nx, k, 8)."""
    c = po.camera(*cam, near=near, far=far)
    gen = po.gen_rays4 if four else po.gen_rays1
    return np.stack([np.stack([gen(c, film_w, film_h, nx, ny, px, py) for px in range(nx)]) for py in range(ny)])


# ---- ray batches ----------------------------------------------------------------------
def extreme_rays(rng, n, mn, mx):
    """Raw rays (not normalised): huge and overflowing direction components
    (travorder distances +-inf and NaN), denormal and zero components, far
    origins, NaN / inf components, origins on split planes, +-FLT_MIN
    components, and odd [tmin, tmax] ranges."""
    mn, mx = np.asarray(mn, F), np.asarray(mx, F)
    c = (mn + mx) / 2
    ext = (mx - mn) / 2
    rays = np.zeros((n, 8), F)
    for i in range(n):
        o = (c + rng.uniform(-1.2, 1.2, 3) * ext).astype(F)
        d = rng.normal(0, 1, 3).astype(F)
        k = i % 12
        if k == 0:
            d = (d / np.abs(d).max() * 3e38).astype(F)
        elif k == 1:
            d[rng.integers(0, 3)] = F(2e38) * np.sign(d[0] + 0.1)
        elif k == 2:
            d[rng.integers(0, 3)] = F(1e-41)
        elif k == 3:
            d[:] = 0
            d[rng.integers(0, 3)] = 1e-40
        elif k == 4:
            o = (o * F(1e20)).astype(F)
            d = (c - o).astype(F)
        elif k == 5:
            d[rng.integers(0, 3)] = np.nan
        elif k == 6:
            o[rng.integers(0, 3)] = np.inf
        elif k == 7:
            d = (d * F(1e19)).astype(F)
        elif k == 8:  # zero components (replaced by FLT_MIN in AABB3D::isect)
            d[rng.integers(0, 3)] = 0.0
            if i % 24 == 8:
                d[rng.integers(0, 3)] = -0.0
        elif k == 9:  # +-FLT_MIN components
            d[rng.integers(0, 3)] = F(FLT_MIN) * rng.choice(np.array([-1.0, 1.0]))
        elif k == 10:  # origin on a split plane of the root or of a child
            a = rng.integers(0, 3)
            h = (mx[a] - mn[a]) / F(2)
            o[a] = [mn[a], mn[a] + h, (mn[a] + h) + h, mn[a] + h / F(2)][rng.integers(0, 4)]
        # k == 11: plain
        rays[i, :3], rays[i, 3:6] = o, d
        rays[i, 6], rays[i, 7] = [(0.0, FLT_MAX), (-np.inf, np.inf), (0.5, 0.1), (0.0, 0.2), (0.3, 2.5)][i % 5]
    return rays


def random_rays(rng, n, mn, mx):
    """Normalised rays from around the box, some with zero components or along
    an axis, some with their own [tmin, tmax]."""
    mn, mx = np.asarray(mn, F), np.asarray(mx, F)
    c = (mn + mx) / 2
    ext = (mx - mn) / 2
    o = (c + rng.uniform(-1.3, 1.3, (n, 3)) * ext).astype(F)
    d = rng.normal(0, 1, (n, 3)).astype(F)
    zero = rng.random(n) < 0.15
    d[zero, rng.integers(0, 3, zero.sum())] = 0.0
    ax = rng.random(n) < 0.05
    d[ax] = 0.0
    d[ax, rng.integers(0, 3, ax.sum())] = 1.0
    rays = np.zeros((n, 8), F)
    for i in range(n):
        tmin = 0.0 if i % 4 else float(rng.uniform(0, 0.3))
        tmax = FLT_MAX if i % 7 else float(rng.uniform(0.5, 3))
        rays[i] = po.make_ray(o[i], d[i], tmin, tmax)
    return rays


def batch_rays(seed, n, mn, mx):
    """n rays: half random, half of the extreme families."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.concatenate([random_rays(rng, n // 2, mn, mx),
                                                extreme_rays(rng, n - n // 2, mn, mx)]))


def node_boxes(rng, n, mn, mx, levels=8):
    """n node boxes by split()'s arithmetic from the root, random level and path."""
    lo = np.tile(np.asarray(mn, F), (n, 1))
    hi = np.tile(np.asarray(mx, F), (n, 1))
    lv = rng.integers(0, levels, n)
    for step in range(levels - 1):
        go = (lv > step)[:, None]
        h = ((hi - lo) / F(2.0)).astype(F)
        m = rng.integers(0, 2, (n, 3)).astype(F)
        cmn = (lo + m * h).astype(F)
        cmx = (cmn + h).astype(F)
        lo = np.where(go, cmn, lo).astype(F)
        hi = np.where(go, cmx, hi).astype(F)
    return np.ascontiguousarray(np.concatenate([lo, hi], axis=1))


def box_ray_pairs(seed, mn, mx, nbox=200, per_box=20):
    """About nbox * per_box (box, ray) pairs: every box with random and extreme
    rays drawn around itself (so many hit, graze or start on its planes)."""
    rng = np.random.default_rng(seed)
    boxes = node_boxes(rng, nbox, mn, mx)
    bb, rr = [], []
    for b in boxes:
        grow = (b[3:] - b[:3]) * F(0.5)
        r = np.concatenate([random_rays(rng, per_box // 2, b[:3] - grow, b[3:] + grow),
                            extreme_rays(rng, per_box - per_box // 2, b[:3], b[3:])])
        bb.append(np.tile(b, (len(r), 1)))
        rr.append(r)
    return np.ascontiguousarray(np.concatenate(bb)), np.ascontiguousarray(np.concatenate(rr))


# ---- probes -------------------------------------------------------------------------
def scene_probes(mn, mx, n=8, seed=11):
    """n probes inside the box: some small, some large enough to be hit often."""
    mn, mx = np.asarray(mn, F), np.asarray(mx, F)
    c, ext = (mn + mx) / 2, (mx - mn) / 2
    rng = np.random.default_rng(seed)
    o = (c + rng.uniform(-0.7, 0.7, (n, 3)) * ext).astype(F)
    r = (np.array([0.1, 0.05, 0.3, 0.1, 0.2, 0.02, 0.15, 0.25] * (n // 8 + 1), F)[:n] * ext.min() * F(2)).astype(F)
    return np.ascontiguousarray(np.concatenate([o, r[:, None]], axis=1))


def unit_dirs(seed, n):
    d = np.random.default_rng(seed).normal(0, 1, (n, 3))
    return np.ascontiguousarray((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F))


def sg_pairs(seed, n):
    """n SG pairs (n, 7) {a, d, s} and n directions: unit and unnormalised
    axes, sharpness 0, tiny, usual and very large."""
    rng = np.random.default_rng(seed)

    def side():
        a = rng.uniform(0, 2, (n, 3)).astype(F)
        d = unit_dirs(rng.integers(1 << 30), n)
        s = rng.choice(np.array([0.0, 1e-6, 0.5, 10.0, 10.0, 37.5, 1e4, 1e30], F), n).astype(F)
        return np.ascontiguousarray(np.concatenate([a, d, s[:, None]], axis=1))
    return side(), side(), unit_dirs(seed + 1, n)


_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = ctypes.c_float
_libm.expf.argtypes = [ctypes.c_float]
PI = F(3.1415926535897932384626)  # jql::pi, a float (VRT/graphics_math.h:23)


def _expf(x):
    return np.array([_libm.expf(float(v)) for v in np.asarray(x, F).reshape(-1)], F).reshape(np.shape(x))


def _dot(a, b):
    """jql::dot: sum{0}; sum += p_k * q_k."""
    s = np.zeros(len(a), F)
    for k in range(3):
        s = (s + a[:, k] * b[:, k]).astype(F)
    return s


def sg_model(lhs, rhs, dirs):
    """SG::eval, SG::integral, prod and inner_prod (VRT/voxel_octree.cc:503-528)
    in float32, one rounding per operation, the C library's expf.
    SG::integral's unqualified exp on a float is the float overload, as its
    std::expf neighbours are."""
    la, ld, ls = lhs[:, 0:3], lhs[:, 3:6], lhs[:, 6]
    ra, rd, rs = rhs[:, 0:3], rhs[:, 3:6], rhs[:, 6]
    with np.errstate(all="ignore"):
        ev = (la * _expf(ls * (_dot(dirs, ld) - F(1)))[:, None]).astype(F)
        tmp = (F(1.0) - _expf((F(-2.0) * ls).astype(F))).astype(F)
        integral = (((F(2) * PI) * (la / ls[:, None]).astype(F)).astype(F) * tmp[:, None]).astype(F)
        um = ((ls[:, None] * ld).astype(F) + (rs[:, None] * rd).astype(F)).astype(F)
        lm = (ls + rs).astype(F)
        d = (um / lm[:, None]).astype(F)
        dl = np.sqrt(_dot(d, d)).astype(F)
        pa = ((la * ra).astype(F) * _expf(lm * (dl - F(1)))[:, None]).astype(F)
        pd = (d / np.sqrt(_dot(d, d))[:, None]).astype(F)  # SG's constructor normalises
        prod = np.concatenate([pa, pd, (lm * dl).astype(F)[:, None]], axis=1)
        uml = np.sqrt(_dot(um, um)).astype(F)
        expo = ((_expf(((uml - ls).astype(F) - rs).astype(F))[:, None] * la).astype(F) * ra).astype(F)
        other = (F(1.0) - _expf((F(-2.0) * uml).astype(F))).astype(F)
        inner = ((((F(2.0) * PI) * expo).astype(F) * other[:, None]).astype(F) / uml[:, None]).astype(F)
    return {"eval": ev, "integral": integral, "prod": prod, "inner": inner}


# ---- trace()'s combine (VRT/main.cc:10-30) ---------------------------------------------
def sky(rays):
    """float t = 0.5 * (ray.d.y + 1.0) in double, narrowed; lerp(a, b, t) =
    a + (b - a) * t in float32 (VRT/graphics_math.h lerp)."""
    t = (0.5 * (np.asarray(rays, F)[:, 4].astype(np.float64) + 1.0)).astype(F)
    a, b = np.ones(3, F), np.array([0.6, 0.8, 1.0], F)
    return (a[None, :] + (b - a)[None, :] * t[:, None]).astype(F)


def combine_trace(rays, hit, visible, albedo, indirect, direct):
    """albedo * (indirect + direct) on a visible hit, albedo on an invisible
    one, the sky on a miss, one float32 rounding per operation."""
    with np.errstate(all="ignore"):
        lit = (albedo * (indirect + direct).astype(F)).astype(F)
    out = np.where((visible == 1)[:, None], lit, albedo)
    return np.where((hit == 1)[:, None], out, sky(rays)).astype(F)


def film_samples(nx, ny):
    """(x, y) of every sample of a film in pixel order, four per pixel."""
    y, x = np.divmod(np.arange(nx * ny), nx)
    return np.ascontiguousarray(np.repeat(np.stack([x, y], axis=1), 4, axis=0).astype(np.int32))
