"""vrt_probe_irradiance on the host: the light a scene's probes send to a point
-- the mean, over the probes of the point's leaf, of the sum over their 14
stored lobes of inner_prod(lobe, SG{lobe_a, normal, lobe_s}) -- against a numpy
restatement built from the scene's own queries: the descent over
tree.nodes()' boxes (child 4 (p.x > c.x) + 2 (p.y > c.y) + (p.z > c.z), c =
(min + max) * .5f), the lists of tree.probe_leaves(), reference_gi_cases.
sg_model's inner_prod (pinned to the reference's compiled code by
tests/test_reference_gi_host.py), float32 sums in list and lobe order, and the
division by the count.

Scene: the committed scene_proxy.npz with the 8 probes and the depth (5) of
tests/golden/ref_gi_probes.npz, host-only.  Bar: identity -- counts equal,
every float equal in its bits, NaN matching NaN.  No GPU is used.

tests/test_sg_probe_gpu.py imports the scene, the stored SGs, the queries and
the restatement from here."""
import ctypes as C

import numpy as np
import pytest

import voxelraytrace20190722_amd as vrt
from voxelraytrace20190722_amd import _ffi
from conftest import golden

import ref_gi_record as rec
import reference_gi_cases as rc

F = np.float32
LOBE = ((vrt.SG_COSINE_AMPLITUDE,) * 3, vrt.SG_COSINE_SHARPNESS)
LEAF_BIT = np.uint32(0x80000000)


def scene():
    """(scene, probes (8, 4), depth) of the recorded probe scene."""
    sd = rec.scene()
    zp = golden("ref_gi_probes.npz")
    assert str(zp["scene_sha"]) == str(rec.scene_sha(sd))
    return sd, np.ascontiguousarray(zp["scene_probes"], F), int(zp["probe_depth"])


def stored_sgs(nprobe, seed=3, odd=2):
    """nprobe x 14 records: the 14 normalised dirs_, sharpness 10, seeded
    amplitudes; probe `odd` gets a lobe of sharpness 0, one of 1e4 and an
    axis that is not unit."""
    rng = np.random.default_rng(seed)
    d = vrt.PROBE_DIRS.astype(F)
    d = (d / np.sqrt(rc._dot(d, d))[:, None]).astype(F)
    sgs = {"a": rng.uniform(0, 2, (nprobe, 14, 3)).astype(F), "d": np.tile(d, (nprobe, 1, 1)),
           "s": np.full((nprobe, 14), 10, F)}
    sgs["s"][odd, 0], sgs["s"][odd, 1] = 0.0, 1e4
    sgs["d"][odd, 2] = (sgs["d"][odd, 2] * F(1.7)).astype(F)
    return sgs


def sg_records(sgs):
    return np.ascontiguousarray(np.concatenate([sgs["a"], sgs["d"], sgs["s"][:, :, None]], axis=2))


def leaf_centres(tree, vox):
    """The centres of max-depth leaves from their voxel ids and the root box
    (well inside the leaf: nothing here depends on their last bits)."""
    mn, mx = (np.asarray(v, np.float64) for v in tree.root_box)
    g = 1 << (tree.max_depth - 1)
    ijk = np.stack([vox & 1023, (vox >> 10) & 1023, (vox >> 20) & 1023], axis=1).astype(np.float64)
    return (mn + (ijk + 0.5) * (mx - mn) / g).astype(F)


def queries(tree, seed=19):
    """About 2,000 (hit_p, normal): the centres of every leaf with two or more
    probes and of 200 leaves with one, 1,000 random points in the root box,
    the root centre and points with a coordinate exactly on an internal node's
    centre plane, points just outside each face of the root box, a NaN
    coordinate, a zero normal and normals that are not unit."""
    rng = np.random.default_rng(seed)
    mn, mx = tree.root_box
    vox, cnt, _ = tree.probe_leaves()
    one = np.flatnonzero(cnt == 1)
    pick = np.concatenate([np.flatnonzero(cnt >= 2), rng.choice(one, min(200, len(one)), replace=False)])
    pts = [leaf_centres(tree, vox[pick])]
    inside = (mn + rng.uniform(0, 1, (1000, 3)) * (mx - mn)).astype(F)
    inside = np.minimum(np.maximum(inside, mn), mx)
    pts.append(inside)
    # centre planes: the root's and those of 200 internal nodes, one coordinate
    # exactly on the plane and the others inside that node
    box, a, _ = tree.nodes()
    internal = np.flatnonzero((a & LEAF_BIT) == 0)
    planes = [((box[0, :3] + box[0, 3:]) * F(.5)).astype(F)]
    for i in np.concatenate([[0], rng.choice(internal, min(200, len(internal)), replace=False)]):
        c = ((box[i, :3] + box[i, 3:]) * F(.5)).astype(F)
        for k in range(3):
            p = (box[i, :3] + rng.uniform(0.05, 0.95, 3) * (box[i, 3:] - box[i, :3])).astype(F)
            p[k] = c[k]
            planes.append(p)
    pts.append(np.array(planes, F))
    # on and just outside each face
    faces = []
    c = ((mn + mx) * F(.5)).astype(F)
    for k in range(3):
        for edge, away in ((mn[k], -np.inf), (mx[k], np.inf)):
            on, out = c.copy(), c.copy()
            on[k], out[k] = edge, np.nextafter(F(edge), F(away))
            faces += [on, out]
    pts.append(np.array(faces, F))
    p = np.ascontiguousarray(np.concatenate(pts))
    nrm = rng.normal(0, 1, p.shape).astype(F)
    nrm[::3] = (nrm[::3] / np.linalg.norm(nrm[::3], axis=1, keepdims=True)).astype(F)  # a third are unit
    # the leaves with most probes once more: a NaN coordinate, a zero normal
    top = leaf_centres(tree, vox[np.argsort(-cnt.astype(np.int64), kind="stable")[:2]])
    p = np.concatenate([p, top])
    nrm = np.concatenate([nrm, np.ones((2, 3), F)])
    p[-2, 1] = np.nan
    nrm[-1] = 0.0
    return np.ascontiguousarray(p), np.ascontiguousarray(nrm)


def descend(tree, p):
    """Per point: the probe list of its leaf ([] outside the root box, in a
    leaf above max depth or without probes)."""
    box, a, _ = tree.nodes()
    vox, cnt, lists = tree.probe_leaves()
    start = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    table = {int(v): lists[start[j]:start[j + 1]] for j, v in enumerate(vox)}
    n = len(p)
    with np.errstate(invalid="ignore"):
        inside = np.all((p >= box[0, :3]) & (p <= box[0, 3:]), axis=1)
    idx = np.zeros(n, np.int64)
    ijk = np.zeros((n, 3), np.int64)
    depth = np.ones(n, np.int64)
    for _ in range(tree.max_depth):
        go = inside & ((a[idx] & LEAF_BIT) == 0)
        if not go.any():
            break
        c = ((box[idx, :3] + box[idx, 3:]) * F(.5)).astype(F)
        with np.errstate(invalid="ignore"):
            bit = (p > c).astype(np.int64)
        child = 4 * bit[:, 0] + 2 * bit[:, 1] + bit[:, 2]
        idx = np.where(go, a[idx].astype(np.int64) + child, idx)
        ijk = np.where(go[:, None], 2 * ijk + bit, ijk)
        depth += go
    assert np.all(~inside | ((a[idx] & LEAF_BIT) != 0))
    out = []
    for i in range(n):
        v = int(ijk[i, 0] | (ijk[i, 1] << 10) | (ijk[i, 2] << 20))
        out.append(table.get(v, []) if inside[i] and depth[i] == tree.max_depth else [])
    return out


def restate(tree, sgs, p, nrm, lobe=LOBE):
    """(rgb (n, 3), count (n,)) of the contract, in numpy."""
    lists = descend(tree, p)
    count = np.array([len(l) for l in lists], np.int32)
    recs = sg_records(sgs)
    n = len(p)
    with np.errstate(all="ignore"):
        qd = (nrm / np.sqrt(rc._dot(nrm, nrm))[:, None]).astype(F)  # SG's constructor
    q = np.concatenate([np.tile(np.asarray(lobe[0], F), (n, 1)), qd, np.full((n, 1), lobe[1], F)], axis=1)
    lhs, rhs, owner = [], [], []
    for i, l in enumerate(lists):
        for k in l:
            lhs.append(recs[k])
            rhs.append(np.tile(q[i], (14, 1)))
            owner += [i] * 14
    rgb = np.zeros((n, 3), F)
    if not owner:
        return rgb, count
    lhs, rhs, owner = np.concatenate(lhs), np.concatenate(rhs), np.array(owner)
    inner = rc.sg_model(lhs, rhs, np.zeros((len(lhs), 3), F))["inner"]
    first = np.searchsorted(owner, np.arange(n))  # owner is sorted: a point's terms are contiguous
    acc = np.zeros((n, 3), F)
    with np.errstate(all="ignore"):
        for t in range(14 * int(count.max())):
            on = t < 14 * count
            acc[on] = (acc[on] + inner[first[on] + t]).astype(F)
        lit = count > 0
        rgb[lit] = (acc[lit] / count[lit].astype(F)[:, None]).astype(F)
    return rgb, count


class Case:
    """A host-only probe scene with stored SGs, its queries and the
    restatement's answers, computed once."""

    def __init__(self, probes=None, sgs=None):
        self.sd, base, self.depth = scene()
        self.probes = base if probes is None else probes
        self.tree = vrt.VoxelOctree(self.sd, self.depth, device=-1, probes=self.probes)
        self.sgs = stored_sgs(len(self.probes)) if sgs is None else sgs
        self.tree.probe_sgs = self.sgs
        self.p, self.nrm = queries(self.tree)
        self.rgb, self.count = restate(self.tree, self.sgs, self.p, self.nrm)


@pytest.fixture(scope="module")
def case():
    return Case()


def test_fixture_tree_is_the_one_the_queries_were_chosen_for(case):
    _, cnt, _ = case.tree.probe_leaves()
    assert [int((cnt == k).sum()) for k in (1, 2, 3)] == [513, 31, 3] and cnt.max() == 3


def test_host_call_equals_the_restatement(case):
    c = case.count
    # the condition on the query set, before anything is compared
    assert (c == 3).sum() >= 3 and (c == 2).sum() >= 20 and (c == 1).sum() >= 100 and (c == 0).sum() >= 100
    assert 1800 <= len(case.p) <= 2200
    rgb, count = case.tree.probe_irradiance(case.p, case.nrm, counts=True)
    assert np.array_equal(count, c)
    assert rc.same_f32(rgb, case.rgb), rc.diff_count(rgb, case.rgb)
    assert not rc.bits(rgb[c == 0]).any()                      # +0 where no probe lights the point
    assert np.isnan(rgb[-1]).all() and c[-1] >= 2              # the zero normal
    assert c[-2] == 0                                          # the NaN coordinate is outside
    lit = np.isfinite(rgb).all(axis=1) & (c > 0)
    assert lit.sum() >= 200 and (rgb[lit] > 0).all()
    # count = NULL: the same rgb
    assert rc.same_f32(case.tree.probe_irradiance(case.p, case.nrm), case.rgb)


def test_the_lobe_is_the_callers(case):
    sel = np.flatnonzero(case.count > 0)[:60]
    p, nrm = case.p[sel], case.nrm[sel]
    lobe = ((0.3, 1.0, 2.5), 7.25)
    want, cnt = restate(case.tree, case.sgs, p, nrm, lobe)
    rgb, count = case.tree.probe_irradiance(p, nrm, lobe[0], lobe[1], counts=True)
    assert np.array_equal(count, cnt) and rc.same_f32(rgb, want)
    assert not rc.same_f32(want, case.rgb[sel])


def test_the_stored_sgs_are_read_at_call_time(case):
    sel = np.flatnonzero(case.count > 0)[:40]
    half = {"a": (case.sgs["a"] * F(0.5)).astype(F), "d": case.sgs["d"], "s": case.sgs["s"]}
    try:
        case.tree.probe_sgs = half
        want, _ = restate(case.tree, half, case.p[sel], case.nrm[sel])
        assert rc.same_f32(case.tree.probe_irradiance(case.p[sel], case.nrm[sel]), want)
    finally:
        case.tree.probe_sgs = case.sgs


def test_n_zero_one_and_refusals(case):
    L = vrt.lib()
    la = np.array(LOBE[0], F)
    lap = la.ctypes.data_as(_ffi.f32p)
    assert case.tree.probe_irradiance(np.zeros((0, 3), F), np.zeros((0, 3), F)).shape == (0, 3)
    assert L.vrt_probe_irradiance(case.tree.h, None, 0, lap, LOBE[1], None, None) == 0
    i = int(np.flatnonzero(case.count == 3)[0])
    rgb, count = case.tree.probe_irradiance(case.p[i:i + 1], case.nrm[i:i + 1], counts=True)
    assert count[0] == 3 and rc.same_f32(rgb, case.rgb[i:i + 1])
    isects = np.ascontiguousarray(np.concatenate([case.p[:4], case.nrm[:4]], axis=1))
    ip = isects.ctypes.data_as(C.POINTER(_ffi.ISect))
    out = np.full((4, 3), 7, F)
    op = out.ctypes.data_as(_ffi.f32p)
    for call in (lambda: L.vrt_probe_irradiance(None, ip, 4, lap, LOBE[1], op, None),
                 lambda: L.vrt_probe_irradiance(case.tree.h, None, 4, lap, LOBE[1], op, None),
                 lambda: L.vrt_probe_irradiance(case.tree.h, ip, 4, None, LOBE[1], op, None),
                 lambda: L.vrt_probe_irradiance(case.tree.h, ip, 4, lap, LOBE[1], None, None),
                 lambda: L.vrt_probe_irradiance(case.tree.h, ip, -1, lap, LOBE[1], op, None)):
        assert call() == _ffi.VRT_E_INVALID
    assert np.all(out == 7)
    # the device call on a host-only scene
    with pytest.raises(vrt.VrtError) as e:
        case.tree.probe_irradiance_device(isects.ctypes.data, 4, out.ctypes.data)
    assert e.value.status == _ffi.VRT_E_NODEVICE and np.all(out == 7)


def test_scene_without_probes_is_refused(case):
    tree = vrt.VoxelOctree(case.sd, 3, device=-1)
    with pytest.raises(vrt.VrtError) as e:
        tree.probe_irradiance(case.p[:4], case.nrm[:4])
    assert e.value.status == _ffi.VRT_E_INVALID and "no probes" in str(e.value)
    with pytest.raises(vrt.VrtError) as e:
        tree.probe_irradiance_device(1, 4, 1)  # refused before any pointer is looked at
    assert e.value.status == _ffi.VRT_E_INVALID
