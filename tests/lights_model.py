"""A float32 model of a light map built from several coloured lights
(vrt_lightmap_build_lights): the reference's light block (VRT/main.cc:80-97)
run once per light, light after light, into one map, then one
cone_trace_init_filter (VRT/voxel_octree.cc:190-214).

The oracle's ora_lightmap clears its map on every call and shades under a
white light, so it cannot be the yardstick for several lights.  This model
takes from the oracle only what does not depend on the light list -- the rays
(gen_rays4), each sample's hit, voxel and normal (ray_march) and get_diffuse
under white (shade) -- and restates the rest in numpy float32, one rounding
per operation.  test_lights_model.py pins it to the oracle's own unfiltered
and filtered maps for one white light, bit for bit.

No GPU is needed; nothing here calls the library under test."""
import numpy as np

import pyoracle as po

f32 = np.float32

# VoxelOctree::illum_d (VRT/voxel_octree.cc:19-20): +x, +y, +z, -x, -y, -z
ILLUM_D = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], f32)


class ModelLight:
    """cam = (fov, eye, spot, up) as po.camera takes it; film = (nx, ny), 1 x 1
    physical; color = get_diffuse's colour argument."""

    def __init__(self, cam, film, color=(1.0, 1.0, 1.0)):
        self.cam, self.film, self.color = cam, (int(film[0]), int(film[1])), tuple(float(c) for c in color)

    def white(self):
        return ModelLight(self.cam, self.film)


def canonical_rays(cam, nx, ny):
    """The light pass's rays in the canonical single-threaded order: render_mt
    task t = tx*8 + ty (VRT/camera.h:50-56) of ptx x pty pixels, pixels
    row-major, gen_rays4's samples 0..3.  (n, 8) float32."""
    c = po.camera(*cam)
    ptx, pty = nx // 8, ny // 8
    out = []
    for t in range(64):
        tx, ty = t // 8, t % 8
        for py in range(pty * ty, pty * ty + pty):
            for px in range(ptx * tx, ptx * tx + ptx):
                out.append(po.gen_rays4(c, 1.0, 1.0, nx, ny, px, py))
    return np.concatenate(out) if out else np.zeros((0, 8), f32)


_samples = {}


def light_samples(osc, key, light):
    """Per hit sample of one light, in canonical order: (leaf key, normal,
    get_diffuse under white).  Cached per (scene key, camera, film)."""
    k = (key, light.cam, light.film)
    if k not in _samples:
        rays = canonical_rays(light.cam, *light.film)
        if len(rays) == 0:
            _samples[k] = (np.zeros(0, np.uint64), np.zeros((0, 3), f32), np.zeros((0, 3), f32))
        else:
            m = osc.ray_march(rays)
            hit = m["hit"] == 1
            leaf = (np.uint64(osc.max_depth) << np.uint64(32)) | m["voxel"][hit].astype(np.uint64)
            _samples[k] = (leaf, m["normal"][hit].astype(f32), osc.shade(rays)[hit].astype(f32))
        for a in _samples[k]:
            a.setflags(write=False)
    return _samples[k]


def accumulate(osc, key, lights):
    """leaf->illum[i] += clamp(dot(illum_d[i], n), 0, 1) * get_diffuse(isect,
    ray, color), sample by sample, light by light.  Returns (hits, leaf keys
    (sorted, unique), illum (n, 6, 3) float32, per-light leaf key arrays)."""
    leaf, nrm, col, per_light = [], [], [], []
    for l in lights:
        lf, n, white = light_samples(osc, key, l)
        c = np.asarray(l.color, f32)
        leaf.append(lf)
        nrm.append(n)
        # get_diffuse = (albedo * tmp) * color: one float32 multiplication per component
        col.append((white * c[None, :]).astype(f32))
        per_light.append(np.unique(lf))
    leaf, nrm, col = np.concatenate(leaf), np.concatenate(nrm), np.concatenate(col)
    hits = len(leaf)
    # dot = (d.x*n.x + d.y*n.y) + d.z*n.z, clamped to [0, 1]
    d = ILLUM_D
    dot = ((d[None, :, 0] * nrm[:, None, 0] + d[None, :, 1] * nrm[:, None, 1]).astype(f32)
           + d[None, :, 2] * nrm[:, None, 2]).astype(f32)
    coeff = np.minimum(np.maximum(dot, f32(0)), f32(1)).astype(f32)
    term = (col[:, None, :] * coeff[:, :, None]).astype(f32)  # muls(illum, coeff)
    keys, inv = np.unique(leaf, return_inverse=True)
    L = np.zeros((len(keys), 6, 3), f32)
    # each leaf's chain is sequential; the chains of different leaves are
    # independent, so step j adds every leaf's j-th sample at once
    order = np.argsort(inv, kind="stable")
    starts = np.searchsorted(inv[order], np.arange(len(keys)))
    pos = np.arange(hits) - starts[inv[order]]
    by_pos = np.argsort(pos, kind="stable")
    cuts = np.searchsorted(pos[by_pos], np.arange(int(pos.max()) + 2 if hits else 1))
    for j in range(len(cuts) - 1):
        s = order[by_pos[cuts[j]:cuts[j + 1]]]
        L[inv[s]] = (L[inv[s]] + term[s]).astype(f32)
    return hits, keys, L, per_light


def _coords(key):
    return (key >> np.uint64(32), key & np.uint64(1023), (key >> np.uint64(10)) & np.uint64(1023),
            (key >> np.uint64(20)) & np.uint64(1023))


def lightmap(osc, key, lights, filter=True, node_keys=None, nonempty_keys=None):
    """(hits, (node keys, coverage, illum)) as lightmap_nodes returns them,
    for the lights in the order given.  filter=False: the sums alone
    (coverage all zero, as the oracle's unfiltered map).  A probe scene has
    more nodes than the oracle's triangle octree and counts a leaf that holds
    only probes as non-empty: its sorted node keys and the keys of its
    non-empty leaves are then passed in (the light pass itself is
    visible-only, so the samples are the triangle scene's)."""
    hits, lkeys, L, _ = accumulate(osc, key, lights)
    nkeys = osc.lightmap_nodes()[0] if node_keys is None else np.asarray(node_keys, np.uint64)
    at = {int(k): i for i, k in enumerate(nkeys)}
    cov = np.zeros(len(nkeys), f32)
    ill = np.zeros((len(nkeys), 6, 3), f32)
    for k, v in zip(lkeys, L):
        ill[at[int(k)]] = v
    if not filter:
        return hits, (nkeys, cov, ill)
    if nonempty_keys is None:
        nonempty = {(int(osc.max_depth) << 32) | int(v) for v in osc.leaves()[0]}
    else:
        nonempty = {int(k) for k in nonempty_keys}
    dep, x, y, z = (a.astype(np.int64) for a in _coords(nkeys))
    for d in sorted(set(dep.tolist()), reverse=True):
        for i in np.flatnonzero(dep == d):
            kids = []
            for c in range(8):
                bx, by, bz = c >> 2, (c >> 1) & 1, c & 1
                kids.append(((d + 1) << 32) | (2 * x[i] + bx) | ((2 * y[i] + by) << 10) | ((2 * z[i] + bz) << 20))
            if kids[0] in at:  # internal: the sequential sum of children 0..7 from zero, then / 8
                acc, c_acc = np.zeros((6, 3), f32), f32(0)
                for kk in kids:
                    acc = (acc + ill[at[kk]]).astype(f32)
                    c_acc = f32(c_acc + cov[at[kk]])
                ill[i] = (acc / f32(8)).astype(f32)
                cov[i] = f32(c_acc / f32(8))
            elif int(nkeys[i]) in nonempty:
                cov[i] = 1
            else:
                cov[i] = 0
                ill[i] = 0
    return hits, (nkeys, cov, ill)


def shared_leaves(osc, key, lights):
    """Leaves hit by every one of the lights."""
    sets = accumulate(osc, key, lights)[3]
    out = sets[0]
    for s in sets[1:]:
        out = np.intersect1d(out, s)
    return len(out)


def order_sensitive(osc, key, lights_a, lights_b):
    """Nodes whose unfiltered illum differs in bits between two orders."""
    a = lightmap(osc, key, lights_a, filter=False)[1][2]
    b = lightmap(osc, key, lights_b, filter=False)[1][2]
    return int((a.view(np.uint32) != b.view(np.uint32)).any(axis=(1, 2)).sum())


# ---- the test lights on proxy(0.25, 2) ------------------------------------
UP = (0.0, 1.0, 0.0)


def issue_lights(to_radian):
    """A, B, C, Z of the issue; to_radian: the library's degree conversion."""
    A = ModelLight((to_radian(60), (1.0, 10.0, 1.0), (0.0, 0.0, 0.0), UP), (64, 64), (1.0, 1.0, 1.0))
    B = ModelLight((to_radian(75), (-4.0, 6.0, 2.5), (0.5, 0.5, 0.0), UP), (40, 72), (0.25, 1.5, 0.7))
    C = ModelLight((to_radian(50), (3.0, 2.0, -1.0), (0.0, 1.0, 0.0), UP), (48, 24), (2.0, 0.125, 0.6))
    Z = ModelLight(C.cam, (7, 64), (1.0, 1.0, 1.0))
    return A, B, C, Z

