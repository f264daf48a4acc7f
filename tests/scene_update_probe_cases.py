"""Scenes and helpers shared by test_scene_update_probes_host.py and
test_scene_update_probes_gpu.py: scene_update_cases.rigid's motion restated so
that the same float32 rotation and shift move the probe centres, the root-box
rule over vertices and then probe faces with the sign of a zero, "the moved
soup" (scene_soup.npz and probe_set under that motion, with radii that kill
one probe, wake one and grow the outside one), and small soups whose root box
is decided by a probe face (zero ties, infinite faces).  A helper module: it
holds no tests."""
import numpy as np

import voxelraytrace20190722_amd as vrt

import scene_update_cases as uc
from test_probe_scene_host import _soup, probe_set

f32 = np.float32
RADIUS_FACTORS = np.array((1.5, 1, 0, 1, 1, 2, 1), np.float32)
INFO = ("nodes", "internal", "leaves", "nonempty_leaves", "tri_refs", "max_depth", "device")


def motion(angle=0.37, shift=(0.25, -0.125, 0.5)):
    """uc.rigid's rotation about (1, 2, 3) and its translation, every
    operation in float32 -> (R, t)."""
    ax = np.array((1, 2, 3), np.float32)
    ax /= np.sqrt((ax * ax).sum(dtype=np.float32), dtype=np.float32)
    c, s = f32(np.cos(angle)), f32(np.sin(angle))
    K = np.array(((0, -ax[2], ax[1]), (ax[2], 0, -ax[0]), (-ax[1], ax[0], 0)), np.float32)
    R = (np.eye(3, dtype=np.float32) + s * K + (f32(1) - c) * (K @ K)).astype(np.float32)
    return R, np.asarray(shift, np.float32)


def rigid_probes(probes, angle=0.37, shift=(0.25, -0.125, 0.5)):
    """The probes under uc.rigid's motion: centres (o @ R.T + t) in float32,
    radii unchanged."""
    R, t = motion(angle, shift)
    p = np.array(probes, np.float32).reshape(-1, 4)
    p[:, :3] = (p[:, :3] @ R.T + t).astype(np.float32)
    return np.ascontiguousarray(p)


def root_rule(pos, probes):
    """build_tree's root box of a probe scene: uc.root_rule over the vertices,
    then every probe's {o - r, o + r} (one float32 operation each) in probe
    order through std::min / std::max -- of equal extremes the first in voxel
    order keeps its bits, so a vertex beats a probe face and probe k beats
    probe k + 1."""
    mn, mx = uc.root_rule(pos)
    with np.errstate(all="ignore"):
        for p in np.asarray(probes, np.float32).reshape(-1, 4):
            lo, hi = (p[:3] - p[3]).astype(np.float32), (p[:3] + p[3]).astype(np.float32)
            for k in range(3):
                if lo[k] < mn[k]:
                    mn[k] = lo[k]
                if mx[k] < hi[k]:
                    mx[k] = hi[k]
    return mn, mx


class MovedSoup:
    """scene_soup.npz (2,500 triangles) with probe_set, and both under
    uc.rigid's default motion; the moved radii x RADIUS_FACTORS, probe 6's set
    to 0.07 x the smallest extent of the moved triangles' box: probe 2 dies,
    probe 6 comes alive, the outside probe 5 grows.  (sd: another scene made
    to move the same way.)"""

    def __init__(self, sd=None):
        self.sd = _soup() if sd is None else sd
        self.probes = probe_set(self.sd)
        self.pos, self.nrm = uc.rigid(self.sd.pos, self.sd.nrm)
        self.moved = uc.with_arrays(self.sd, self.pos, self.nrm)
        p = rigid_probes(self.probes)
        p[:, 3] = (p[:, 3] * RADIUS_FACTORS).astype(np.float32)
        v = self.pos.reshape(-1, 3)
        p[6, 3] = f32(0.07) * (v.max(axis=0) - v.min(axis=0)).min()
        self.moved_probes = np.ascontiguousarray(p)


def tie_triangles():
    """24 small triangles with every x >= 0.01: a zero face of a probe, or a
    zero vertex put in by the caller, is the minimum of x."""
    p = uc.spread(24, 11).reshape(-1, 3, 3)
    p[..., 0] = np.abs(p[..., 0]) + f32(0.01)
    return p.reshape(-1, 9)


HALF = (0.5, 0.5, 0.5, 0.5)         # faces {+0, 1} on every axis
POINT = (-0.0, 0.5, 0.5, 0.0)       # r = 0 at x = -0: faces {-0 - 0, -0 + 0} = {-0, +0}


def root_cases():
    """name -> (pos, probes, check) with check(root_min, root_max) the case's
    own claim beside the restated rule."""
    def min_x_zero(neg):
        return lambda mn, mx: mn[0] == 0 and bool(np.signbit(mn[0])) == neg

    vert = tie_triangles()
    vert[3, 3] = f32(-0.0)              # the x of triangle 3's second vertex
    return {
        "probe +0 before probe -0": (tie_triangles(), np.array([HALF, POINT], np.float32), min_x_zero(False)),
        "probe -0 before probe +0": (tie_triangles(), np.array([POINT, HALF], np.float32), min_x_zero(True)),
        "vertex -0 before probe +0": (vert, np.array([HALF], np.float32), min_x_zero(True)),
        "face +inf": (tie_triangles(), np.array([(3e38, 0.5, 0.5, 3e38)], np.float32),
                      lambda mn, mx: mx[0] == np.inf and np.isfinite(mn).all()),
        "face -inf": (tie_triangles(), np.array([(-3e38, 0.5, 0.5, 3e38)], np.float32),
                      lambda mn, mx: mn[0] == -np.inf and np.isfinite(mx).all()),
    }


def flat(x):
    if isinstance(x, dict):
        return [a for k in sorted(x) for a in flat(x[k])]
    if isinstance(x, (tuple, list)):
        return [a for v in x for a in flat(v)]
    if isinstance(x, np.ndarray):
        return [uc.bits(x)]
    return [np.asarray(x)]


def host_queries(tree):
    """What a host-only probe scene answers: info, root box bits, nodes,
    leaves, probe info, probe leaves, record format."""
    return {
        "info": [np.asarray([getattr(tree.info, f) for f in INFO])],
        "root": flat(tree.root_box),
        "nodes": flat(tree.nodes()),
        "leaves": flat(tree.leaves()),
        "probe info": flat(tree.probe_info()),
        "probe leaves": flat(tree.probe_leaves()),
        "format": flat(tree.ref_record_bytes),
    }


def same(got, want, what):
    assert list(got) == list(want)
    for k in want:
        assert len(got[k]) == len(want[k]), (what, k)
        for a, b in zip(got[k], want[k]):
            assert a.shape == b.shape and np.array_equal(a, b), (what, k)


def random_probes(n, seed=23):
    """n probes with centres in the unit cube and radii <= 0.05."""
    r = np.random.RandomState(seed)
    p = r.rand(n, 4).astype(np.float32)
    p[:, 3] *= f32(0.05)
    return np.ascontiguousarray(p)


def probe_scene(sd, depth, probes, **kw):
    return vrt.VoxelOctree(sd, depth, probes=np.ascontiguousarray(probes, np.float32), **kw)
