"""Expected values for the tests of light probes as scene voxels
(vrt_scene_create_probes, the even_invisible march, trace() on a probe
scene): float32 restatements of the reference, one numpy float32 operation
per operation of the reference, with the oracle's primitives for the
triangle side (tri_box_overlap, aabb_isect, sort8, intersect_triangle3,
first_min).  A helper module: it holds no tests."""
import ctypes as C

import numpy as np

import probe_cases as pc
import pyoracle as po

f32 = np.float32
FLT_MAX = f32(np.finfo(np.float32).max)
LEAF = 0x80000000


# ---- LightProbe::is_overlap / isect ---------------------------------------
def is_overlap(probe, box):
    """LightProbe::is_overlap (VRT/voxel_octree.cc:567-586): probe {o, r},
    box {min, max}."""
    o, r = np.asarray(probe[:3], np.float32), f32(probe[3])
    c1, c2 = np.asarray(box[:3], np.float32), np.asarray(box[3:6], np.float32)
    with np.errstate(all="ignore"):
        dist_squared = f32(r * r)
        for k in range(3):
            if o[k] < c1[k]:
                v = f32(o[k] - c1[k])
                dist_squared = f32(dist_squared - f32(v * v))
            elif o[k] > c2[k]:
                v = f32(o[k] - c2[k])
                dist_squared = f32(dist_squared - f32(v * v))
    return bool(dist_squared > 0)


def _dot(a, b):
    s = f32(0)
    for k in range(3):
        s = f32(s + f32(a[k] * b[k]))
    return s


def _std_min(a, b):
    return b if b < a else a


def _std_max(a, b):
    return b if a < b else a


def sphere_ray_isect(probe, ray):
    """jql::sphere_ray_isect + quadratic_solver (VRT/graphics_math.h:
    1105-1126, 1175-1206) -> t or None.  tmin / tmax are not consulted."""
    so, sr = np.asarray(probe[:3], np.float32), f32(probe[3])
    ro, rd = np.asarray(ray[:3], np.float32), np.asarray(ray[3:6], np.float32)
    with np.errstate(all="ignore"):
        a = f32(1)
        tmp3 = (ro - so).astype(np.float32)
        b = f32(f32(2) * _dot(tmp3, rd))
        c = f32(_dot(tmp3, tmp3) - f32(sr * sr))
        delta = f32(f32(b * b) - f32(f32(f32(4) * a) * c))
        if delta < 0:
            return None
        if b > 0:
            tmp = f32(f32(-b) - np.sqrt(delta))
        else:
            tmp = f32(f32(-b) + np.sqrt(delta))
        t1_ = f32(tmp / f32(f32(2) * a))
        t2_ = f32(f32(f32(2) * c) / tmp)
        t1, t2 = _std_min(t1_, t2_), _std_max(t1_, t2_)
        if t2 < 0:
            return None
        if t1 >= 0:
            return f32(t1)
        if t2 >= 0:
            return f32(t2)
        return None


def probe_isect(probe, ray, prev_hit):
    """LightProbe::isect (VRT/voxel_octree.cc:546-554): `*isect = ISect{ray.o +
    t * ray.d, isect->hit - o_}` reads the ISect's hit point before the
    assignment, and ISect's constructor (VRT/graphics_math.h:1138-1142)
    normalises its second argument -> (t, hit, normal) or None."""
    t = sphere_ray_isect(probe, ray)
    if t is None:
        return None
    ro, rd = np.asarray(ray[:3], np.float32), np.asarray(ray[3:6], np.float32)
    with np.errstate(all="ignore"):
        hit = (ro + t * rd).astype(np.float32)
        nrm = pc.normalize((np.asarray(prev_hit, np.float32) - np.asarray(probe[:3], np.float32)).astype(np.float32))
    return t, hit, nrm


# ---- ray_march_init over triangles, then probes ------------------------------
def root_box(pos, probes):
    """AABB{} merged with every voxel's get_aabb() in voxel order
    (VRT/voxel_octree.cc:70-72): min / max are exact, so the order does not
    matter for the triangles; the probes' {o - r, o + r} are float32."""
    pos = np.asarray(pos, np.float32).reshape(-1, 3, 3)
    mn, mx = np.full(3, FLT_MAX, np.float32), np.full(3, -FLT_MAX, np.float32)
    if len(pos):
        mn, mx = np.minimum(mn, pos.min(axis=(0, 1))), np.maximum(mx, pos.max(axis=(0, 1)))
    for p in np.asarray(probes, np.float32).reshape(-1, 4):
        mn = np.minimum(mn, (p[:3] - p[3]).astype(np.float32))
        mx = np.maximum(mx, (p[:3] + p[3]).astype(np.float32))
    return np.concatenate([mn, mx]).astype(np.float32)


def child_box(box, i):
    """split() (VRT/voxel_octree.cc:27-39)."""
    with np.errstate(all="ignore"):
        half = ((box[3:] - box[:3]) / f32(2)).astype(np.float32)
        mask = np.array([1 if i & 4 else 0, 1 if i & 2 else 0, 1 if i & 1 else 0], np.float32)
        mn = (box[:3] + mask * half).astype(np.float32)
        return np.concatenate([mn, (mn + half).astype(np.float32)])


class Build:
    """insert() / split() (VRT/voxel_octree.cc:27-65) level by level over the
    mixed voxel list (voxel v < ntri: triangle v, else probe v - ntri), to
    `max_depth`.  A voxel reaches a node iff it overlaps the node and all its
    ancestors; a node above max_depth is split iff some voxel reaches it, and a
    leaf at max_depth lists the voxels that reach it, in voxel order -- what
    the sequential insertion produces.  Nodes are numbered like the flattened
    tree: breadth first, an internal node's 8 children contiguous, the blocks
    in the order of their parents.  `at(depth)` gives the tree of a smaller
    max_depth, which is a prefix of this one.

    Triangle::is_overlap is the oracle's tri_box_overlap.  It is asked only
    for triangles whose box comes within 1e-3 of the root's extent of the
    node's box: triBoxOverlap's own first test rejects a triangle whose
    vertices all lie beyond the box on one axis, and float32 rounding moves
    that comparison by ~1e-7 of the extent, far below the margin."""

    def __init__(self, pos, probes, max_depth):
        self.pos = np.ascontiguousarray(np.asarray(pos, np.float32).reshape(-1, 9))
        self.probes = np.asarray(probes, np.float32).reshape(-1, 4)
        self.ntri, self.max_depth = len(self.pos), max_depth
        tri = self.pos.reshape(-1, 3, 3)
        self.tmn, self.tmx = tri.min(axis=1), tri.max(axis=1)
        root = root_box(self.pos, self.probes)
        self.margin = f32(1e-3) * (root[3:] - root[:3]).max()
        self._tbo = po.oracle().ora_tri_box_overlap
        self._base = self.pos.ctypes.data
        # per level: boxes, the voxels reaching each node (overlap already applied)
        self.levels = []
        boxes = [root]
        cand = [np.arange(self.ntri + len(self.probes))]
        for depth in range(1, max_depth + 1):
            reach = [self._overlapping(b, c) for b, c in zip(boxes, cand)]
            self.levels.append((boxes, reach))
            nb, nc = [], []
            for b, r in zip(boxes, reach):
                if len(r):
                    for i in range(8):
                        nb.append(child_box(b, i))
                        nc.append(r)
            boxes, cand = nb, nc
            if not boxes:
                break

    def _overlapping(self, box, cand):
        tris = cand[cand < self.ntri]
        if len(tris):
            near = np.all((self.tmx[tris] >= box[:3] - self.margin) & (self.tmn[tris] <= box[3:] + self.margin), axis=1)
            tris = tris[near]
        with np.errstate(all="ignore"):
            c = np.ascontiguousarray(((box[:3] + box[3:]) * f32(0.5)).astype(np.float32))
            h = np.ascontiguousarray(((box[3:] - box[:3]) / f32(2)).astype(np.float32))
        cp, hp = c.ctypes.data_as(po.f32p), h.ctypes.data_as(po.f32p)
        keep = [t for t in tris.tolist() if self._tbo(cp, hp, C.cast(self._base + 36 * t, po.f32p)) == 1]
        keep += [v for v in cand[cand >= self.ntri].tolist() if is_overlap(self.probes[v - self.ntri], box)]
        return np.array(keep, np.int64)

    def at(self, depth):
        """The tree of max_depth = depth: boxes (n, 6), word a (first child, or
        LEAF), per node its triangle list and its probe list (leaves at
        `depth` only), node depth."""
        boxes, a, tris, prs, dep = [], [], [], [], []
        for l in range(1, depth + 1):
            if l > len(self.levels):
                break
            lb, reach = self.levels[l - 1]
            boxes += lb
            dep += [l] * len(lb)
            for r in reach:
                if l == depth:
                    a.append(LEAF)
                    tris.append(r[r < self.ntri])
                    prs.append(r[r >= self.ntri] - self.ntri)
                else:
                    a.append(None if len(r) else LEAF)
                    tris.append(r[:0])
                    prs.append(r[:0])
        # children blocks: internal nodes in index order own the next blocks
        nxt = 1
        for i, w in enumerate(a):
            if w is None:
                a[i] = nxt
                nxt += 8
        assert nxt == len(a)
        return np.array(boxes, np.float32), np.array(a, np.uint32), tris, prs, np.array(dep)


def leaf_lists(a, keys, voxel, count, items):
    """Per node its list from a (voxel ids sorted, counts, concatenated
    lists) triple as vrt_scene_leaves / vrt_scene_probe_leaves return it."""
    out = [np.zeros(0, np.int64)] * len(a)
    at = dict(zip((int(v) for v in voxel), range(len(voxel))))
    start = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    for i in np.flatnonzero((a & np.uint32(LEAF)) != 0):
        j = at.get(int(keys[i]) & 0xFFFFFFFF)
        if j is not None:
            out[i] = np.asarray(items[start[j]:start[j + 1]], np.int64)
    return out


def tree_lists(tree):
    """(boxes, a, triangle list per node, probe list per node) of a library
    tree: its nodes with its leaves() and probe_leaves().  Lists live in the
    leaves at max_depth only, where a voxel id names one node."""
    box, a, _ = tree.nodes()
    keys = pc.node_keys(a)
    deep = (keys >> np.uint64(32)) == np.uint64(tree.max_depth)
    tl = leaf_lists(a, keys, *tree.leaves())
    pl = leaf_lists(a, keys, *tree.probe_leaves())
    for i in np.flatnonzero(~deep):
        tl[i] = pl[i] = np.zeros(0, np.int64)
    return box, a, tl, pl


# ---- gi::ray_march(root, ray, .., even_invisible) ----------------------------
class Walker:
    """ray_march / ray_march_isect (VRT/voxel_octree.cc:99-188) over a tree
    given as arrays, with Triangle::isect (:438-460) and LightProbe::isect."""

    def __init__(self, sd, probes, box, a, tris, prs, node_vox):
        self.pos = np.asarray(sd.pos, np.float32).reshape(-1, 9)
        self.nrm = pc.normalize(np.asarray(sd.nrm, np.float32).reshape(-1, 3, 3))  # Triangle::Triangle
        self.probes = np.asarray(probes, np.float32).reshape(-1, 4)
        self.box, self.a, self.tris, self.prs, self.node_vox = box, a, tris, prs, node_vox
        self.ntri = len(self.pos)
        with np.errstate(all="ignore"):
            self.center = ((box[:, :3] + box[:, 3:]) * f32(0.5)).astype(np.float32)
        # the oracle's intersect_triangle3 on the widened vertices (Triangle::isect's
        # double copies), called through pointers made once per triangle list
        self._pos64 = np.ascontiguousarray(self.pos.astype(np.float64))
        self._v0 = self._pos64[:, 0:3]
        self._e1, self._e2 = self._pos64[:, 3:6] - self._v0, self._pos64[:, 6:9] - self._v0
        self._mt = po.oracle().ora_intersect_triangle3
        self._tuv = [C.c_double() for _ in range(3)]

    def candidates(self, tris, ray):
        """The triangles of a long list that the oracle has to be asked about,
        in list order.  intersect_triangle3 (VRT/raytri.cc:197-249) accepts
        only |det| > 1e-6 and barycentrics inside the triangle; the same
        double-precision formulas over the whole list at once discard the
        triangles that miss those tests by more than 1e-6 (|det| by a factor
        of two), a margin ~1e9 times the rounding of the formulas.  The
        oracle decides every triangle that is left."""
        if len(tris) <= 16 or not np.all(np.isfinite(ray[:6])):
            return tris
        o, d = ray[:3].astype(np.float64), ray[3:6].astype(np.float64)
        e1, e2, v0 = self._e1[tris], self._e2[tris], self._v0[tris]
        with np.errstate(all="ignore"):
            p = np.cross(d, e2)
            det = (e1 * p).sum(axis=1)
            tv = o - v0
            u = (tv * p).sum(axis=1) / det
            v = (np.cross(tv, e1) * d).sum(axis=1) / det
            keep = (np.abs(det) > 0.5e-6) & (u >= -1e-6) & (v >= -1e-6) & (u + v <= 1 + 1e-6)
        return tris[keep | ~np.isfinite(u) | ~np.isfinite(v)]

    def tri_isect(self, t, ray):
        od = np.ascontiguousarray(ray[:6].astype(np.float64))
        base, ob = self._pos64.ctypes.data + 72 * t, od.ctypes.data
        ptrs = [C.cast(a, po.f64p) for a in (ob, ob + 24, base, base + 24, base + 48)]
        r = self._mt(*ptrs, *[C.byref(x) for x in self._tuv])
        if r != 1:
            return None
        dt, du, dv = (x.value for x in self._tuv)
        with np.errstate(all="ignore"):
            u, v = pc.clamp01(f32(du)), pc.clamp01(f32(dv))
            w = pc.clamp01(f32(f32(f32(1) - u) - v))
            n = self.nrm[t]
            ntmp = ((n[0] * w + n[1] * u).astype(np.float32) + n[2] * v).astype(np.float32)
            return (ray[:3] + f32(dt) * ray[3:6]).astype(np.float32), pc.normalize(ntmp)

    def leaf(self, node, ray, even_invisible, isect_hit):
        """ray_march_isect: records (hit, normal, depth, voxel) in list order;
        `isect_hit` is the caller's ISect::hit, which every successful record
        overwrites -> (winner record or None, stats)."""
        recs = []
        for t in self.candidates(self.tris[node], ray):
            r = self.tri_isect(int(t), ray)
            if r is not None:
                isect_hit = r[0]
                recs.append((r[0], r[1], int(t), isect_hit))
        if even_invisible:
            for k in self.prs[node]:
                prev = isect_hit
                r = probe_isect(self.probes[int(k)], ray, prev)
                if r is not None:
                    isect_hit = r[1]
                    recs.append((r[1], r[2], self.ntri + int(k), prev))
        if not recs:
            return None, None
        with np.errstate(all="ignore"):
            depth = [np.sqrt(pc.dot(h - ray[:3], h - ray[:3])) for h, _, _, _ in recs]
        win = recs[po.first_min(np.array(depth, np.float32))]
        kinds = {v >= self.ntri for _, _, v, _ in recs}
        return win, {"both": len(kinds) == 2, "prev_nonzero": bool(np.any(win[3] != 0))}

    def travorder(self, node, ray):
        with np.errstate(all="ignore"):
            c0 = int(self.a[node])
            dist = [pc.dot(ray[3:6], (self.center[c0 + ci] - ray[:3]).astype(np.float32)) for ci in range(8)]
        return [c0 + int(ci) for ci in po.sort8(np.array(dist, np.float32))]

    def march(self, ray, even_invisible=True):
        """-> (hit dict or None, stats of the winning leaf)."""
        ray = np.asarray(ray, np.float32)
        zero = np.zeros(3, np.float32)  # trace()'s `ISect isect{}`
        if not po.aabb_isect(self.box[0], ray):
            return None, None
        stack = [[0]] if self.a[0] & LEAF else [self.travorder(0, ray)]
        while stack:
            node = stack[-1].pop(0)
            if not stack[-1]:
                stack.pop()
            if node != 0 and not po.aabb_isect(self.box[node], ray):
                continue
            if not (self.a[node] & LEAF):
                stack.append(self.travorder(node, ray))
                continue
            win, st = self.leaf(node, ray, even_invisible, zero)
            if win is not None:
                return {"tri": win[2], "voxel": int(self.node_vox[node]), "hit_p": win[0], "normal": win[1],
                        "node": node}, st
        return None, None

    def batch(self, rays, even_invisible=True):
        n = len(rays)
        out = {"hit": np.zeros(n, np.int32), "tri": np.full(n, -1, np.int32),
               "voxel": np.full(n, 0xFFFFFFFF, np.uint32), "hit_p": np.zeros((n, 3), np.float32),
               "normal": np.zeros((n, 3), np.float32), "node": np.full(n, -1, np.int64),
               "both": np.zeros(n, bool), "prev_nonzero": np.zeros(n, bool)}
        for i in range(n):
            h, st = self.march(rays[i], even_invisible)
            if h is None:
                continue
            out["hit"][i] = 1
            for k in ("tri", "voxel", "hit_p", "normal", "node"):
                out[k][i] = h[k]
            out["both"][i], out["prev_nonzero"][i] = st["both"], st["prev_nonzero"]
        return out


# ---- cone_trace_init_filter ---------------------------------------------------
def init_filter(a, nonempty, leaf_illum):
    """cone_trace_init_filter (VRT/voxel_octree.cc:190-213) over node arrays:
    a leaf with a non-empty list has coverage 1 and keeps its illum, an empty
    one coverage 0 and zero illum; an internal node sums its children in
    order from zero and divides by 8.  leaf_illum (n, 6, 3)."""
    n = len(a)
    cov = np.zeros(n, np.float32)
    ill = np.zeros((n, 6, 3), np.float32)
    for i in range(n - 1, -1, -1):  # children follow their parent
        if a[i] & LEAF:
            if nonempty[i]:
                cov[i] = 1
                ill[i] = leaf_illum[i]
            continue
        c0 = int(a[i])
        cs, isum = f32(0), np.zeros((6, 3), np.float32)
        for c in range(8):
            cs = f32(cs + cov[c0 + c])
            isum = (isum + ill[c0 + c]).astype(np.float32)
        cov[i] = f32(cs / f32(8))
        ill[i] = (isum / f32(8)).astype(np.float32)
    return cov, ill
