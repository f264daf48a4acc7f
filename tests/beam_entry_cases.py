"""Host restatement of the beam entry (k_unit_entry and the hand-off in
ray_march, vrt_kernels.hip) in numpy float32, every operation
rounded and none contracted: the pre-pass over a unit's 64 rays, the per-ray
walk it must agree with, and the units of tests/test_beam_entry_host.py and
tests/test_beam_entry_gpu.py.  Not a test module."""
import numpy as np

import chain_order_cases as cc

F = np.float32
LEAF = 0x80000000
ENTRY_WORDS = 16
ENTRY_MAX = 7
ENTRY_NONE = 0xFFFFFFFF
CHAIN_BIT = 0x100
FLT_MAX = F(3.4028234663852886e38)
FLT_MIN = F(1.1754943508222875e-38)
STACK = 10
POPC = np.array([bin(x).count("1") for x in range(256)], np.int32)


class Tree:
    """What the walk reads of a scene: the node records, their triangle boxes
    (march_nodes in vrt_host.cpp, restated) and the scene constants."""

    def __init__(self, vo, sd):
        box, a, b = vo.nodes()
        self.bmin = np.ascontiguousarray(box[:, 0:3], F)
        self.bmax = np.ascontiguousarray(box[:, 3:6], F)
        self.a, self.b = a, b
        self.rmin, self.rmax = self.bmin[0].copy(), self.bmax[0].copy()
        self.wmin = self._spacing()
        dev = np.asarray(vo.chain_spacing, F)  # zeros on a host-only scene
        assert np.all(self.wmin > 0) and (np.all(dev == 0) or np.array_equal(dev, self.wmin))
        ext = F(np.max(self.rmax - self.rmin))
        self.lb_center = F(0.5) * (self.rmin + self.rmax)
        self.lb_reach = F(16.0) * ext
        self.tmn, self.tmx = self._tri_boxes(vo, sd, ext)

    def _spacing(self):
        """chain_spacing (vrt_host.cpp): per axis the smallest child-centre
        spacing over the internal nodes, exact in double, rounded down."""
        i = (self.a & LEAF) == 0
        a0, b, c = cc.planes(self.bmin[i], self.bmax[i])
        c0, c1 = (a0 + b) * F(.5), (b + c) * F(.5)
        assert np.all((c0 >= self.rmin) & (c1 <= self.rmax))
        w = np.min(c1.astype(np.float64) - c0.astype(np.float64), 0)
        f = w.astype(F)
        return np.where(f.astype(np.float64) > w, np.nextafter(f, F(0)), f).astype(F)

    def _tri_boxes(self, vo, sd, ext):
        n = self.a.shape[0]
        leaf = (self.a & LEAF) != 0
        nref = np.where(leaf, self.a & ~np.uint32(LEAF), 0).astype(np.int64)
        # leaves() lists the non-empty leaves by (voxel id, node index): the
        # voxel id packs the path's child bits per axis (vox_of, vrt_host.cpp)
        xyz = np.zeros((n, 3), np.int64)
        for i in np.nonzero(~leaf)[0]:  # parents precede their children
            c = int(self.a[i])
            ci = np.arange(8)
            xyz[c:c + 8] = (xyz[i] << 1) | np.stack([(ci >> 2) & 1, (ci >> 1) & 1, ci & 1], 1)
        vox = xyz[:, 0] | (xyz[:, 1] << 10) | (xyz[:, 2] << 20)
        ne = np.nonzero(nref > 0)[0]
        ne = ne[np.lexsort((ne, vox[ne]))]
        lvox, cnt, tris = vo.leaves()
        assert np.array_equal(lvox, vox[ne]) and np.array_equal(cnt, nref[ne]) and int(nref.sum()) == len(tris)
        first = np.concatenate([[0], np.cumsum(nref[ne])[:-1]]).astype(np.int64)
        p = sd.pos[tris].reshape(-1, 3, 3).astype(np.float64)
        rl, rh = p.min(1), p.max(1)
        lo = np.full((n, 3), np.inf)
        hi = np.full((n, 3), -np.inf)
        lo[ne] = np.minimum.reduceat(rl, first, 0)
        hi[ne] = np.maximum.reduceat(rh, first, 0)
        for i in range(n - 1, -1, -1):  # children follow their parent
            if not leaf[i]:
                c = int(self.a[i])
                lo[i] = lo[c:c + 8].min(0)
                hi[i] = hi[c:c + 8].max(0)
        tmn, tmx = self.bmin.copy(), self.bmax.copy()
        eps = np.ldexp(np.float64(ext), -16)
        has = lo[:, 0] <= hi[:, 0]
        has[0] = False
        with np.errstate(all="ignore"):
            fl = (lo - eps).astype(F)
            fl = np.where(fl.astype(np.float64) > lo - eps, np.nextafter(fl, F(-np.inf)), fl)
            fh = (hi + eps).astype(F)
            fh = np.where(fh.astype(np.float64) < hi + eps, np.nextafter(fh, F(np.inf)), fh)
        tmn[has], tmx[has] = fl[has], fh[has]
        return tmn, tmx

    def lbok(self, o):
        return bool(np.all(np.abs(o - self.lb_center) <= self.lb_reach))


def dinv_of(d):
    with np.errstate(all="ignore"):
        return (F(1.0) / np.where(d == 0, FLT_MIN, d)).astype(F)


def rays_ok(o, d, di):
    """fast_ok && fin_ok per ray for tmin = +0, tmax = FLT_MAX."""
    ad = np.abs(d)
    ok = np.all(np.abs(o) < F(2.0 ** 60))
    per = np.all((d == 0) | ((ad >= FLT_MIN) & (ad < F(2.0 ** 64))), 1)
    return ok & per & np.all(np.abs(di) <= F(2.0 ** 64), 1)


def _mul(plane, o, dlo, dhi):
    c = (plane - o).astype(F)
    a, b = c * dlo, c * dhi
    return np.minimum(a, b), np.maximum(a, b)


def _verdict(t0lo, t0hi, t1lo, t1hi):
    """0 missed for certain, 1 hit for certain, 2 uncertain."""
    if t0hi <= t1lo:
        return 1
    if t0lo > t1hi:
        return 0
    return 2


def beam_box(bmin, bmax, o, dlo, dhi, fold):
    alo, ahi = _mul(bmin, o, dlo, dhi)
    blo, bhi = _mul(bmax, o, dlo, dhi)
    t0lo, t0hi = np.max(np.minimum(alo, blo)), np.max(np.minimum(ahi, bhi))
    t1lo, t1hi = np.min(np.maximum(alo, blo)), np.min(np.maximum(ahi, bhi))
    if fold:
        t0lo, t0hi = max(t0lo, F(0)), max(t0hi, F(0))
    return _verdict(t0lo, t0hi, t1lo, t1hi)


def beam_expand(bmin, bmax, o, dlo, dhi, content):
    """-> (every content child certain, mask of the children hit for certain)."""
    a0, b, c = cc.planes(bmin, bmax)
    ta, tb, tc = _mul(a0, o, dlo, dhi), _mul(b, o, dlo, dhi), _mul(c, o, dlo, dhi)
    # [bound][axis][half]
    nr = [np.stack([np.minimum(ta[j], tb[j]), np.minimum(tb[j], tc[j])], -1) for j in (0, 1)]
    fr = [np.stack([np.maximum(ta[j], tb[j]), np.maximum(tb[j], tc[j])], -1) for j in (0, 1)]
    for j in (0, 1):
        nr[j][2, :] = np.maximum(nr[j][2, :], F(0))
    hm, sure = 0, True
    for i in range(8):
        if not (content >> i) & 1:
            continue
        mx, my, mz = (i >> 2) & 1, (i >> 1) & 1, i & 1
        t0 = [max(nr[j][0, mx], nr[j][1, my], nr[j][2, mz]) for j in (0, 1)]
        t1 = [min(fr[j][0, mx], fr[j][1, my], fr[j][2, mz]) for j in (0, 1)]
        v = _verdict(t0[0], t0[1], t1[0], t1[1])
        sure = sure and v != 2
        hm |= (v == 1) << i
    return sure, hm


def _pack_list(kids):
    w = 0
    for k, ci in enumerate(kids):
        w |= int(ci) << (3 * k)
    return w


def prepass(tree, o, d):
    """k_unit_entry for one unit: o (3,), d (64, 3) -> (the 16-word record,
    committed iterations, committed expansions, stop reason)."""
    rec = np.zeros(ENTRY_WORDS, np.uint32)
    o = np.asarray(o, F)
    d = np.asarray(d, F)
    di = dinv_of(d)
    ok = bool(np.all(rays_ok(o, d, di)))
    s = cc.signs(d)
    n = d.shape[0]
    chain = bool(np.all(cc.criterion(np.tile(tree.rmin, (n, 1)), np.tile(tree.rmax, (n, 1)), np.tile(o, (n, 1)), d,
                                     tree.wmin)))
    dlo, dhi = di.min(0), di.max(0)

    def none(why):
        rec[0] = ENTRY_NONE
        return rec, 0, 0, why

    if not ok:
        return none("not fast")
    if np.any(s != s[0]):
        return none("signs")
    if tree.a[0] & LEAF:
        return none("root leaf")
    if beam_box(tree.rmin, tree.rmax, o, dlo, dhi, True) != 1:
        return none("root")
    cs = int(s[0])

    def order_of(hm):
        k = int(POPC[hm])
        if k <= 1:
            return True, ((hm & -hm).bit_length() - 1) if hm else 0
        if not (chain and cc.CHAIN_VALID[cs, hm]):
            return False, 0
        return True, _pack_list(cc.CHAIN_ORDER[cs, hm][:k])

    lbok = tree.lbok(o)
    sure, hm = beam_expand(tree.rmin, tree.rmax, o, dlo, dhi, int(tree.b[0]))
    good, order = order_of(hm) if sure else (False, 0)
    if not good:
        return none("root expansion")
    sp, cnt, base = 0, int(POPC[hm]), int(tree.a[0])
    stk = []
    iters, nexp, why = 0, 1, "cap"
    while True:
        sp1, cnt1, base1, order1 = sp, cnt, base, order
        if cnt1 == 0:
            if sp1 == 0:
                why = "no hit"
                break
            sp1 -= 1
            base1, w = stk[sp1]
            order1, cnt1 = w & 0xFFFFFF, w >> 24
        ci = order1 & 7
        order1 >>= 3
        cnt1 -= 1
        node = base1 + ci
        tb = beam_box(tree.tmn[node], tree.tmx[node], o, dlo, dhi, False) if lbok else 1
        if tb == 2:
            why = "triangle box"
            break
        push = None
        if tb == 1:
            na, nb = int(tree.a[node]), int(tree.b[node])
            if na & LEAF:
                if na & ~LEAF:
                    why = "leaf"
                    break
            else:
                sure, hm = beam_expand(tree.bmin[node], tree.bmax[node], o, dlo, dhi, nb)
                if not sure:
                    why = "diverge"
                    break
                good, ord_ = order_of(hm)
                if not good:
                    why = "order"
                    break
                if cnt1:
                    if sp1 + 2 > ENTRY_MAX:
                        why = "record full"
                        break
                    push = (base1, order1 | (cnt1 << 24))
                order1, cnt1, base1 = ord_, int(POPC[hm]), na
                nexp += 1
        if push is not None:
            del stk[sp1:]
            stk.append(push)
            sp1 += 1
        sp, cnt, base, order = sp1, cnt1, base1, order1
        iters += 1
    ent = list(stk[:sp])
    if cnt > 0:
        ent.append((base, order | (cnt << 24)))
    rec[0] = len(ent) | (CHAIN_BIT if chain else 0)
    for i, (x, y) in enumerate(ent):
        rec[2 + 2 * i], rec[3 + 2 * i] = x, y
    return rec, iters, nexp, why


def _line_meets(bmin, bmax, o, di):
    a = (bmin - o) * di
    b = (bmax - o) * di
    t0 = np.max(np.minimum(a, b), 1)
    t1 = np.min(np.maximum(a, b), 1)
    return t0 <= t1


def _ray_orders(po, tree, o, d, bmin, bmax, content):
    """Per ray: expand_v2<2>'s hit children in the walk's order -> (packed
    order, count): the chain order where the ray passes the criterion and its
    hit set is a chain, the oracle's sort otherwise."""
    n = d.shape[0]
    ot = np.tile(o, (n, 1))
    hm, dist = cc.expand(bmin, bmax, ot, d)
    hm = hm & content
    cnt = POPC[hm]
    s = cc.signs(d)
    crit = cc.criterion(np.tile(tree.rmin, (n, 1)), np.tile(tree.rmax, (n, 1)), ot, d, tree.wmin)
    use = crit & cc.CHAIN_VALID[s, hm]
    order = cc.CHAIN_ORDER[s, hm].copy()
    rest = np.nonzero(~use & (cnt > 0))[0]
    if len(rest):
        order[rest] = cc.reference_order(po, hm[rest], dist[rest])
    return cc.pack(order, cnt), cnt


def walk_rays(po, tree, o, d, iters):
    """ray_march's finite-slab walk (the root's expansion, then `iters` passes
    of the inner loop) for every ray on its own -> per ray the entry list the
    record must hold, or None for a ray that left the loop (a leaf's triangles,
    the walk's end, a missed root) before that."""
    o = np.asarray(o, F)
    d = np.asarray(d, F)
    n = d.shape[0]
    di = dinv_of(d)
    lbok = tree.lbok(o)
    alive = np.ones(n, bool)
    # the root: aabb_isect in the standard range
    a = (tree.rmin - o) * di
    b = (tree.rmax - o) * di
    t0, t1 = np.max(np.minimum(a, b), 1), np.min(np.maximum(a, b), 1)
    alive &= (t0 <= t1) & ((t0 >= 0) | (t1 >= 0))
    alive &= not (tree.a[0] & LEAF)
    order, cnt = _ray_orders(po, tree, o, d, np.tile(tree.rmin, (n, 1)), np.tile(tree.rmax, (n, 1)),
                             np.uint32(tree.b[0]))
    order = order.astype(np.int64)
    cnt = cnt.astype(np.int64)
    base = np.full(n, int(tree.a[0]), np.int64)
    sp = np.zeros(n, np.int64)
    stk = np.zeros((n, STACK + 1, 2), np.int64)
    r = np.arange(n)
    for _ in range(iters):
        pop = alive & (cnt == 0)
        alive &= ~(pop & (sp == 0))
        pop &= alive
        sp = np.where(pop, sp - 1, sp)
        e = stk[r, np.maximum(sp, 0)]
        base = np.where(pop, e[:, 0], base)
        order = np.where(pop, e[:, 1] & 0xFFFFFF, order)
        cnt = np.where(pop, e[:, 1] >> 24, cnt)
        ci = order & 7
        order = np.where(alive, order >> 3, order)
        cnt = np.where(alive, cnt - 1, cnt)
        node = np.where(alive, base + ci, 0)
        skip = ~_line_meets(tree.tmn[node], tree.tmx[node], o, di) if lbok else np.zeros(n, bool)
        na = tree.a[node].astype(np.int64)
        leaf = (na & LEAF) != 0
        alive &= ~(~skip & leaf & ((na & ~LEAF) != 0))  # a leaf's triangles: out of the loop
        ex = alive & ~skip & ~leaf
        push = ex & (cnt > 0)
        stk[r[push], sp[push], 0] = base[push]
        stk[r[push], sp[push], 1] = order[push] | (cnt[push] << 24)
        sp = np.where(push, sp + 1, sp)
        if np.any(ex):
            i = np.nonzero(ex)[0]
            o2, c2 = _ray_orders(po, tree, o, d[i], tree.bmin[node[i]], tree.bmax[node[i]], tree.b[node[i]])
            order[i], cnt[i], base[i] = o2, c2, na[i]
    out = []
    for k in range(n):
        if not alive[k]:
            out.append(None)
            continue
        ent = [(int(stk[k, j, 0]), int(stk[k, j, 1])) for j in range(sp[k])]
        if cnt[k] > 0:
            ent.append((int(base[k]), int(order[k] | (cnt[k] << 24))))
        out.append(ent)
    return out


def record_entries(rec):
    return [(int(rec[2 + 2 * i]), int(rec[3 + 2 * i])) for i in range(int(rec[0]) & 0xFF)]


# ---- units -----------------------------------------------------------------
def frame_units(cam, film):
    """The 4x4-pixel units of a one-rank frame in unit order (4 * tile +
    quadrant, tiles in raster order): (origin (3,), directions (units, 64, 3)),
    lane = 4 * pixel + sample."""
    ntx, nty = film.nx // 8, film.ny // 8
    px = np.zeros((film.ny, film.nx, 4, 8), F)
    for y in range(film.ny):
        for x in range(film.nx):
            px[y, x] = cam.gen_rays4(film, x, y)
    d = np.zeros((ntx * nty * 4, 64, 3), F)
    for u in range(d.shape[0]):
        k, w = u >> 2, u & 3
        tx, ty = k % ntx, k // ntx
        x0, y0 = tx * 8 + (w & 1) * 4, ty * 8 + (w >> 1) * 4
        d[u] = px[y0:y0 + 4, x0:x0 + 4, :, 3:6].reshape(64, 3)
    assert np.all(px[..., 0:3] == px[0, 0, 0, 0:3]) and np.all(px[..., 6] == 0) and np.all(px[..., 7] == FLT_MAX)
    return px[0, 0, 0, 0:3].copy(), d


def bundle(o, centre, right, up, width):
    """64 unit directions in a 4x4-pixel x 4-sample pattern `width` wide (as
    seen from o at unit distance) about `centre`."""
    sx = np.array([0.125, 0.375, 0.875, 0.625])
    sy = np.array([0.625, 0.125, 0.375, 0.875])
    out = np.zeros((64, 3))
    for lane in range(64):
        p, s = lane >> 2, lane & 3
        u = ((p & 3) + sx[s]) / 4 - .5
        v = ((p >> 2) + sy[s]) / 4 - .5
        out[lane] = centre + width * (u * right + v * up)
    return cc.normalised(out)


def _frame_of(c):
    c = c / np.linalg.norm(c)
    h = np.array([0.0, 1.0, 0.0]) if abs(c[1]) < .9 else np.array([1.0, 0.0, 0.0])
    r = np.cross(c, h)
    r /= np.linalg.norm(r)
    return c, r, np.cross(r, c)


def adversarial_units(tree, seed=7, per=24):
    """(name, origin, 64 directions) bundles about the features the walk's
    decisions turn on.  A unit is about half a leaf wide."""
    rng = np.random.default_rng(seed)
    internal = np.nonzero((tree.a & LEAF) == 0)[0]
    nodes = (tree.bmin[internal], tree.bmax[internal])
    root = (tree.rmin, tree.rmax)
    ext = tree.rmax.astype(np.float64) - tree.rmin
    cen = (tree.rmin.astype(np.float64) + tree.rmax) * .5
    inside = (cen + np.array([0.11, -0.07, 0.05]) * ext).astype(F)
    leaf_w = float(ext.max()) / 64
    out = []

    def add(name, o, centres, width):
        for c in np.asarray(centres, np.float64):
            if not np.all(np.isfinite(c)) or np.linalg.norm(c) == 0:
                continue
            cdir, r, u = _frame_of(c)
            out.append((name, F(o), bundle(o, cdir, r, u, width)))

    # a node's mid planes, edges, corners and centre (family_features aims there)
    bmin, bmax, o, d = cc.family_features(seed, per, nodes, origin=inside, root=root)
    dist = np.linalg.norm((bmin.astype(np.float64) + bmax) * .5 - inside, axis=1)
    for i in range(per):
        add("feature", inside, [d[i]], 0.5 * leaf_w / max(dist[i], leaf_w))
    # near-axis units (the criterion fails)
    bmin, bmax, o, d = cc.family_near_axis(seed + 1, per, nodes, origin=inside, root=root)
    for i in range(per):  # narrower than the small component: one octant
        add("near_axis", inside, [d[i]], 0.25 * float(np.min(np.abs(d[i]))))
    # a direction sign changes inside the unit
    for k in range(3):
        c = np.array([0.6, 0.5, 0.62])
        c[k] = 0.0
        add("sign", inside, [c, -c], 0.02)
    # the eye exactly on a split plane (the root's, then a child's)
    for k in range(3):
        e = inside.copy()
        e[k] = cc.planes(tree.rmin, tree.rmax)[1][k]
        add("on_plane", e, rng.normal(size=(4, 3)), 0.01)
        e2 = e.copy()
        e2[(k + 1) % 3] = cc.planes(tree.rmin, cc.planes(tree.rmin, tree.rmax)[1])[1][(k + 1) % 3]
        add("on_plane", e2, rng.normal(size=(4, 3)), 0.01)
    # an eye outside the root box: towards it, past its silhouette, away
    outside = (cen + np.array([1.3, 0.4, 0.9]) * ext).astype(F)
    add("outside", outside, [cen - outside, tree.rmax.astype(np.float64) - outside,
                             np.array([tree.rmin[0], tree.rmax[1], tree.rmax[2]], np.float64) - outside,
                             outside - cen], 0.01)
    add("outside", outside, (cen + (rng.random((per, 3)) - .5) * 1.4 * ext) - outside, 0.004)
    # an eye beyond lb_reach
    far = (cen + np.array([40.0, 3.0, -2.0]) * float(ext.max())).astype(F)
    add("far", far, (cen + (rng.random((per, 3)) - .5) * ext) - far, 0.0004)
    return out
