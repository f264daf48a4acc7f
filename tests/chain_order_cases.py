"""Host restatement of the walk's child expansion and chain order (expand_v2<2>,
chain_criterion, chain_order2 / chain_order4 in vrt_kernels.hip; DESIGN.md
§4.2), in numpy float32 with every operation rounded and none contracted, and
the input families of tests/test_chain_order_host.py and
tests/test_chain_order_gpu.py.  Not a test module."""
import numpy as np

F = np.float32
U = F(2.0 ** -24)

# the synthetic scene: a non-cubic, off-centre root box and one origin inside it
ROOT_MIN = np.array([-1.37, 0.21, -3.05], F)
ROOT_MAX = np.array([2.11, 1.93, 0.42], F)
ORIGIN = np.array([0.613, 0.977, -1.291], F)
LEVELS = 8  # node levels 0..7


def split_boxes(rng, n, levels=LEVELS):
    """n node boxes by repeated split() arithmetic from the root: level l in
    0..levels-1 (uniform), a random child per step."""
    mn = np.tile(ROOT_MIN, (n, 1))
    mx = np.tile(ROOT_MAX, (n, 1))
    lv = rng.integers(0, levels, n)
    for step in range(levels - 1):
        go = (lv > step)[:, None]
        h = (mx - mn) / F(2.0)
        m = rng.integers(0, 2, (n, 3)).astype(F)
        cmn = mn + m * h
        cmx = cmn + h
        mn = np.where(go, cmn, mn).astype(F)
        mx = np.where(go, cmx, mx).astype(F)
    return mn, mx, lv


def planes(bmin, bmax):
    h = (bmax - bmin) / F(2.0)
    a0 = bmin
    b = bmin + h
    c = b + h
    return a0, b, c


def scene_spacing(levels=LEVELS):
    """ord_wmin of the synthetic scene: per axis the smallest cm[1] - cm[0]
    over every node of levels 0..levels-1 (the axes are independent, so every
    interval of an axis is enumerated), the difference exact in double and
    rounded down to float, as vrt_host.cpp's chain_spacing."""
    w = np.zeros(3, F)
    for k in range(3):
        lo = np.array([ROOT_MIN[k]], F)
        hi = np.array([ROOT_MAX[k]], F)
        best = np.inf
        for _ in range(levels):
            a0, b, c = planes(lo, hi)
            c0 = (a0 + b) * F(.5)
            c1 = (b + c) * F(.5)
            best = min(best, float(np.min(c1.astype(np.float64) - c0.astype(np.float64))))
            lo, hi = np.concatenate([a0, b]), np.concatenate([b, c])
        f = F(best)
        if float(f) > best:
            f = np.nextafter(f, F(0))
        w[k] = f
    assert np.all(w > 0)
    return w


def expand(bmin, bmax, o, d):
    """expand_v2<2> for tmin = +0: hit mask (n,) of the 8 children (all
    present) and the 8 travorder keys (n, 8) float32."""
    with np.errstate(all="ignore"):
        di = (F(1.0) / d).astype(F)
        a0, b, c = planes(bmin, bmax)
        ta = (a0 - o) * di
        tb = (b - o) * di
        tc = (c - o) * di
        nr = np.stack([np.minimum(ta, tb), np.minimum(tb, tc)], -1)  # (n, 3, 2)
        fr = np.stack([np.maximum(ta, tb), np.maximum(tb, tc)], -1)
        nr[:, 2, :] = np.maximum(nr[:, 2, :], F(0.0))
        cm = np.stack([(a0 + b) * F(.5), (b + c) * F(.5)], -1)
        q = d[:, :, None] * (cm - o[:, :, None])
        qx = F(0.0) + q[:, 0, :]
    n = bmin.shape[0]
    hm = np.zeros(n, np.uint32)
    dist = np.zeros((n, 8), F)
    for i in range(8):
        mx_, my_, mz_ = (i >> 2) & 1, (i >> 1) & 1, i & 1
        t0 = np.maximum(np.maximum(nr[:, 0, mx_], nr[:, 1, my_]), nr[:, 2, mz_])
        t1 = np.minimum(np.minimum(fr[:, 0, mx_], fr[:, 1, my_]), fr[:, 2, mz_])
        hm |= (t0 <= t1).astype(np.uint32) << np.uint32(i)
        dist[:, i] = (qx[:, mx_] + q[:, 1, my_]) + q[:, 2, mz_]
    assert dist.dtype == F
    return hm, dist


def criterion(rmin, rmax, o, d, wmin):
    """chain_criterion: gap > 16 * 2^-24 * T and T >= 2^-100, in float32."""
    ad = np.abs(d)
    R = np.maximum(np.abs(rmin - o), np.abs(rmax - o))
    T = F(0.0) + ad[:, 0] * R[:, 0]
    T = T + ad[:, 1] * R[:, 1]
    T = T + ad[:, 2] * R[:, 2]
    g = ad * wmin
    gap = np.minimum(np.minimum(g[:, 0], g[:, 1]), g[:, 2])
    assert T.dtype == F and gap.dtype == F
    return (gap > F(2.0 ** -20) * T) & (T >= F(2.0 ** -100))


def signs(d):
    """The octant mask: bit 2 = x, as the child index."""
    neg = np.signbit(d)
    return (neg[:, 0].astype(np.uint32) << 2) | (neg[:, 1].astype(np.uint32) << 1) | neg[:, 2].astype(np.uint32)


def _chain_tables():
    """From the definition: per (s, hm) whether the hit children are pairwise
    comparable (one canonical code ci ^ s contains the other) and, if so,
    their order by the number of far-side axes."""
    valid = np.zeros((8, 256), bool)
    order = np.full((8, 256, 8), -1, np.int32)
    for s in range(8):
        for hm in range(256):
            kids = [ci for ci in range(8) if (hm >> ci) & 1]
            codes = [ci ^ s for ci in kids]
            ok = all((a & b) == a or (a & b) == b for a in codes for b in codes)
            valid[s, hm] = ok
            if ok:
                assert len(kids) <= 4
                srt = sorted(kids, key=lambda ci: bin(ci ^ s).count("1"))
                assert len({bin(ci ^ s).count("1") for ci in kids}) == len(kids)
                order[s, hm, :len(srt)] = srt
    return valid, order


CHAIN_VALID, CHAIN_ORDER = _chain_tables()


def pack(order, cnt):
    """(n, 8) child lists (-1 padded) -> 3-bit fields, first child in bits 0-2."""
    w = np.zeros(order.shape[0], np.uint32)
    for k in range(8):
        use = (k < cnt) & (order[:, k] >= 0)
        w |= np.where(use, order[:, k], 0).astype(np.uint32) << np.uint32(3 * k)
    return w


def reference_order(po, hm, dist):
    """The oracle's sort8 (libstdc++ std::sort of the 8 Items) per case, the
    hit children kept: (n, 8) -1 padded."""
    import ctypes as C
    n = hm.shape[0]
    dist = np.ascontiguousarray(dist, F)
    full = np.zeros((n, 8), np.int32)
    fn = po.oracle().ora_sort8
    pd = dist.ctypes.data
    pf = full.ctypes.data
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    for i in range(n):
        fn(C.cast(pd + 32 * i, f32p), C.cast(pf + 32 * i, i32p))
    hit = ((hm[:, None] >> full.astype(np.uint32)) & 1).astype(bool)
    out = np.full((n, 8), -1, np.int32)
    pos = np.cumsum(hit, 1) - 1
    r, c = np.nonzero(hit)
    out[r, pos[r, c]] = full[r, c]
    return out


def normalised(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def _boxes(rng, n, nodes):
    """n node boxes: of the synthetic scene, or drawn from `nodes` = (bmin,
    bmax) arrays of a real tree's internal nodes."""
    if nodes is None:
        return split_boxes(rng, n)[:2]
    i = rng.integers(0, nodes[0].shape[0], n)
    return np.ascontiguousarray(nodes[0][i], F), np.ascontiguousarray(nodes[1][i], F)


def _aim(rng, bmin, bmax, o, spread):
    """Directions from o to a random point of the node box scaled by `spread`
    about its centre."""
    c = (bmin.astype(np.float64) + bmax) * .5
    e = bmax.astype(np.float64) - bmin
    t = c + (rng.random(bmin.shape) - .5) * spread * e
    return normalised(t - o)


def family_random(seed, n, nodes=None, origin=ORIGIN, root=(ROOT_MIN, ROOT_MAX)):
    """Rays from the shared origin aimed into or around random nodes."""
    rng = np.random.default_rng(seed)
    bmin, bmax = _boxes(rng, n, nodes)
    o = np.tile(F(origin), (n, 1))
    return bmin, bmax, o, _aim(rng, bmin, bmax, o, 1.5)


def family_near_axis(seed, n, nodes=None, origin=ORIGIN, root=(ROOT_MIN, ROOT_MAX)):
    """The same with one direction component scaled by 10^-3 .. 10^-8."""
    rng = np.random.default_rng(seed)
    bmin, bmax = _boxes(rng, n, nodes)
    o = np.tile(F(origin), (n, 1))
    d = _aim(rng, bmin, bmax, o, 1.5).astype(np.float64)
    k = rng.integers(0, 3, n)
    d[np.arange(n), k] *= 10.0 ** -rng.uniform(3, 8, n)
    return bmin, bmax, o, d.astype(F)


def family_diagonal(seed, n, nodes=None, origin=ORIGIN, root=(ROOT_MIN, ROOT_MAX)):
    """|dx| = |dy| (any dz) and |dx| = |dy| = |dz| exactly, through a point of
    the node, from an origin about one root extent back along the ray."""
    rng = np.random.default_rng(seed)
    bmin, bmax = _boxes(rng, n, nodes)
    sg = rng.choice(np.array([-1.0, 1.0]), (n, 3))
    mag = rng.uniform(0.2, 1.0, (n, 1)).astype(F).astype(np.float64)
    d = sg * mag
    third = rng.random(n) < .5
    d[third, 2] = sg[third, 2] * rng.uniform(0.05, 1.0, third.sum())
    d = d[:, rng.permutation(3)]  # which two axes tie
    d = d.astype(F)
    c = (bmin.astype(np.float64) + bmax) * .5
    e = bmax.astype(np.float64) - bmin
    t = c + (rng.integers(0, 3, (n, 3)) - 1) * .5 * e * rng.choice(np.array([0.0, 0.5, 1.0]), (n, 1))
    ext = float(np.max(F(root[1]) - F(root[0])))
    o = (t - d.astype(np.float64) * rng.uniform(0.15, 0.85, (n, 1)) * ext).astype(F)
    return bmin, bmax, o, d


def family_features(seed, n, nodes=None, origin=ORIGIN, root=(ROOT_MIN, ROOT_MAX)):
    """Rays from the shared origin at the node's corners, edge and face
    centres, its centre and points of its mid planes."""
    rng = np.random.default_rng(seed)
    bmin, bmax = _boxes(rng, n, nodes)
    a0, b, c = planes(bmin, bmax)
    pl = np.stack([a0, b, c], -1)  # (n, 3, 3)
    pick = rng.integers(0, 3, (n, 3))  # per axis: min / mid / max plane
    t = np.take_along_axis(pl, pick[:, :, None], 2)[:, :, 0].astype(np.float64)
    # a third of the cases: leave one axis free in the box (a point on a mid plane or face)
    free = rng.random(n) < 1 / 3
    k = rng.integers(0, 3, n)
    u = bmin[np.arange(n), k] + rng.random(n) * (bmax[np.arange(n), k] - bmin[np.arange(n), k])
    t[free, k[free]] = u[free]
    o = np.tile(F(origin), (n, 1))
    d = normalised(t - o)
    return bmin, bmax, o, d


def family_far(seed, n, nodes=None, origin=ORIGIN, root=(ROOT_MIN, ROOT_MAX)):
    """Rays at random nodes from an origin 100 root extents away, mostly along
    x: near-axis directions whose gap the large R_k must reject."""
    rng = np.random.default_rng(seed)
    bmin, bmax = _boxes(rng, n, nodes)
    ext = float(np.max(F(root[1]) - F(root[0])))
    cen = (F(root[0]).astype(np.float64) + F(root[1])) * .5
    o = np.tile((cen + 100.0 * ext * np.array([1.0, 0.003, -0.002])).astype(F), (n, 1))
    return bmin, bmax, o, _aim(rng, bmin, bmax, o, 1.5)


def evaluate(fam, wmin=None, rmin=ROOT_MIN, rmax=ROOT_MAX):
    """-> dict of the restatement's per-case results for a family."""
    bmin, bmax, o, d = fam
    wmin = scene_spacing() if wmin is None else wmin
    hm, dist = expand(bmin, bmax, o, d)
    s = signs(d)
    cnt = np.array([bin(int(x)).count("1") for x in range(256)], np.int32)[hm]
    n = hm.shape[0]
    return {"hm": hm, "dist": dist, "s": s, "cnt": cnt,
            "crit": criterion(np.tile(rmin, (n, 1)), np.tile(rmax, (n, 1)), o, d, wmin),
            "chain": CHAIN_VALID[s, hm], "order": CHAIN_ORDER[s, hm]}


def device_cases(fam, wmin=None, rmin=ROOT_MIN, rmax=ROOT_MAX):
    """The (n, 21) float32 rows of vrt_device_selftest_chain."""
    bmin, bmax, o, d = fam
    n = bmin.shape[0]
    wmin = scene_spacing() if wmin is None else wmin
    return np.ascontiguousarray(np.concatenate(
        [bmin, bmax, o, d, np.tile(rmin, (n, 1)), np.tile(rmax, (n, 1)), np.tile(wmin, (n, 1))], 1), F)


FAMILIES = {"random": family_random, "near_axis": family_near_axis, "diagonal": family_diagonal,
            "features": family_features, "far": family_far}
