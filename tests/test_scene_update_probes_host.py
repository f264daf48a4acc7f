"""vrt_scene_update_probes on host-only probe scenes (device < 0): the host
build on new vertex arrays and new probes, on the live handle.  After an update
the scene must equal, bit for bit, one freshly created by
vrt_scene_create_probes from the same description with those arrays and
probes; the stored SGs stay.  Also the refusals that need no device, the ctypes
signatures, the root-box rule with probe faces (zero ties, infinite faces)
against its numpy restatement, and one comparison that does not go through the
library's own create: the updated tree against the restated insert()."""
import ctypes as C

import numpy as np
import pytest

import voxelraytrace20190722_amd as vrt
from voxelraytrace20190722_amd import _ffi

import probe_cases as pc
import probe_scene_cases as psc
import scene_update_cases as uc
import scene_update_probe_cases as upc

LEAF = np.uint32(0x80000000)


@pytest.fixture(scope="module")
def ms():
    return upc.MovedSoup()


def host_scene(sd, depth, probes):
    return upc.probe_scene(sd, depth, probes, device=-1)


def holds_probes(tree, sd, depth, probes, what):
    """The library's own host copy of the probes, seen through what it builds:
    an update with probes=None builds from that copy and nothing else."""
    pos = uc.rigid(sd.pos, sd.nrm, angle=0.11, shift=(-0.5, 0.25, 0.125))[0]
    tree.update_probes(pos)
    upc.same(upc.host_queries(tree), upc.host_queries(host_scene(uc.with_arrays(sd, pos), depth, probes)), what)


@pytest.mark.parametrize("depth", [1, 3, 5])
def test_update_equals_fresh_scene(ms, depth):
    tree = host_scene(ms.sd, depth, ms.probes)
    before = upc.host_queries(tree)
    tree.update_probes(ms.pos, ms.nrm, ms.moved_probes)
    fresh = host_scene(ms.moved, depth, ms.moved_probes)
    upc.same(upc.host_queries(tree), upc.host_queries(fresh), f"depth {depth}")
    st = tree.update_stats()
    assert st["total"] > 0 and st["gpu"] == 0 and st["copy_back"] == 0
    # the figures of the moved soup, from the host build
    if depth == 5:
        assert (before["info"][0][0], tree.info.nodes) == (2073, 1977)
        assert [int(v) for v in before["probe info"]] == [7, 97, 116] and tree.probe_info() == (7, 108, 124)
    if depth == 3:
        assert (before["info"][0][0], tree.info.nodes) == (73, 73)
        assert [int(v) for v in before["probe info"]] == [7, 8, 14] and tree.probe_info() == (7, 9, 14)
    listed = set(tree.probe_leaves()[2].tolist())
    assert listed == {0, 1, 3, 4, 5, 6}  # probe 2 died, probe 6 came alive


def test_update_away_and_back(ms):
    orig = host_scene(ms.sd, 3, ms.probes)
    tree = host_scene(ms.sd, 3, ms.probes)
    tree.update_probes(ms.pos, ms.nrm, ms.moved_probes)
    assert not np.array_equal(tree.nodes()[0], orig.nodes()[0])
    tree.update_probes(ms.sd.pos, ms.sd.nrm, ms.probes)
    upc.same(upc.host_queries(tree), upc.host_queries(orig), "back")


def test_only_the_triangles_move(ms):
    tree = host_scene(ms.sd, 3, ms.probes)
    tree.update_probes(ms.pos, ms.nrm)
    upc.same(upc.host_queries(tree), upc.host_queries(host_scene(ms.moved, 3, ms.probes)), "probes=None")


@pytest.mark.parametrize("depth", [3, 5])
def test_new_probes_then_probes_none(ms, depth):
    """The new probes are swapped into the scene's host copy: the next update,
    given none, builds from them and not from the probes of creation."""
    tree = host_scene(ms.sd, depth, ms.probes)
    tree.update_probes(ms.pos, ms.nrm, ms.moved_probes)
    holds_probes(tree, ms.sd, depth, ms.moved_probes, "probes=None after new probes")
    pos = uc.rigid(ms.sd.pos, ms.sd.nrm, angle=0.11, shift=(-0.5, 0.25, 0.125))[0]
    stale = host_scene(uc.with_arrays(ms.sd, pos), depth, ms.probes)
    assert tree.probe_info() != stale.probe_info()  # the two probe sets do not build alike


def test_update_without_normals(ms):
    tree = host_scene(ms.sd, 3, ms.probes)
    tree.update_probes(ms.pos, None, ms.moved_probes)
    upc.same(upc.host_queries(tree), upc.host_queries(host_scene(uc.with_arrays(ms.sd, ms.pos), 3, ms.moved_probes)),
             "nrm=None")


@pytest.mark.parametrize("name", list(upc.root_cases()))
def test_root_box_rule(name):
    pos, probes, check = upc.root_cases()[name]
    mn, mx = upc.root_rule(pos, probes)
    created = host_scene(uc.soup_scene(pos), 3, probes)
    updated = host_scene(uc.soup_scene(uc.spread(pos.shape[0])), 3, upc.random_probes(len(probes)))
    updated.update_probes(pos, None, probes)
    for t in (created, updated):
        assert np.array_equal(uc.bits(t.root_box[0]), uc.bits(mn)), name
        assert np.array_equal(uc.bits(t.root_box[1]), uc.bits(mx)), name
        assert check(*t.root_box), name
    upc.same(upc.host_queries(updated), upc.host_queries(created), name)
    if name == "face +inf":
        assert updated.info.nodes == 17


def test_stored_sgs_survive(ms):
    tree = host_scene(ms.sd, 3, ms.probes)
    rng = np.random.default_rng(3)
    sgs = {"a": rng.random((7, 14, 3), np.float32), "d": rng.random((7, 14, 3), np.float32),
           "s": rng.random((7, 14), np.float32)}
    tree.probe_sgs = sgs
    tree.update_probes(ms.pos, ms.nrm, ms.moved_probes)
    got = tree.probe_sgs
    for k in sgs:
        assert np.array_equal(uc.bits(got[k]), uc.bits(sgs[k])), k


def test_refusals(ms):
    L = _ffi.lib()
    tree = host_scene(ms.sd, 3, ms.probes)
    before = upc.host_queries(tree)
    p = _ffi.ptr(ms.pos, _ffi.f32p)
    pr = ms.moved_probes.ctypes.data_as(C.POINTER(_ffi.Probe))
    assert L.vrt_scene_update_probes(None, p, None, pr) == _ffi.VRT_E_INVALID
    assert L.vrt_scene_update_probes(tree.h, None, None, pr) == _ffi.VRT_E_INVALID
    assert b"null" in L.vrt_last_error()
    assert L.vrt_scene_update_probes_device(None, C.cast(p, C.c_void_p), None, None, None) == _ffi.VRT_E_INVALID
    # a scene without probes: the message names the call to use
    plain = vrt.VoxelOctree(ms.sd, 1, device=-1)
    assert L.vrt_scene_update_probes(plain.h, p, None, None) == _ffi.VRT_E_INVALID
    assert b"vrt_scene_update" in L.vrt_last_error() and b"no light probes" in L.vrt_last_error()
    with pytest.raises(vrt.VrtError) as e:
        plain.update_probes(ms.pos)
    assert e.value.status == _ffi.VRT_E_INVALID
    # ... and vrt_scene_update keeps refusing the probe scene in its own words
    assert L.vrt_scene_update(tree.h, p, None) == _ffi.VRT_E_INVALID
    assert b"is not available on a scene with light probes" in L.vrt_last_error()
    # a bad probe, with its index
    for k, bad in ((4, (np.nan, 0.5, 0.5, 0.1)), (2, (0.5, 0.5, 0.5, -0.25)), (6, (0.5, 0.5, 0.5, np.inf)),
                   (0, (0.5, -np.inf, 0.5, 0.1))):
        q = ms.moved_probes.copy()
        q[k] = bad
        with pytest.raises(vrt.VrtError) as e:
            tree.update_probes(ms.pos, ms.nrm, q)
        assert e.value.status == _ffi.VRT_E_INVALID and f"probe {k}:" in str(e.value)
    # a host-only scene has no device to read from
    assert L.vrt_scene_update_probes_device(tree.h, C.cast(p, C.c_void_p), None, None, None) == _ffi.VRT_E_NODEVICE
    nb = C.c_int64()
    assert L.vrt_scene_device_array(tree.h, 5, None, 0, C.byref(nb)) == _ffi.VRT_E_NODEVICE
    # shapes
    with pytest.raises(ValueError):
        tree.update_probes(ms.pos[:-1])
    with pytest.raises(ValueError):
        tree.update_probes(ms.pos, ms.nrm[:-1])
    with pytest.raises(ValueError):
        tree.update_probes(ms.pos, None, ms.moved_probes[:-1])
    with pytest.raises(ValueError):
        tree.update_probes(ms.pos, None, ms.moved_probes[:, :3])
    upc.same(upc.host_queries(tree), before, "after the refusals")
    holds_probes(tree, ms.sd, 3, ms.probes, "the probes after the refusals")
    tree.update_probes(ms.pos, ms.nrm, ms.moved_probes)
    upc.same(upc.host_queries(tree), upc.host_queries(host_scene(ms.moved, 3, ms.moved_probes)), "the next update")


def test_signatures():
    L = _ffi.lib()
    S = _ffi.SIGNATURES
    assert S["vrt_scene_update_probes"] == (C.c_int, [C.c_void_p, _ffi.f32p, _ffi.f32p, C.POINTER(_ffi.Probe)])
    assert S["vrt_scene_update_probes_device"] == (C.c_int, [C.c_void_p] * 5)
    for name in ("vrt_scene_update_probes", "vrt_scene_update_probes_device"):
        assert getattr(L, name).argtypes == S[name][1] and getattr(L, name).restype == C.c_int


def test_updated_tree_matches_restated_insert(ms):
    """Not through the library's own create: insert() / split() restated
    (probe_scene_cases.Build) on the moved arrays."""
    depth = 3
    tree = host_scene(ms.sd, depth, ms.probes)
    tree.update_probes(ms.pos, ms.nrm, ms.moved_probes)
    wbox, wa, wtris, wprs, _ = psc.Build(ms.pos, ms.moved_probes, depth).at(depth)
    box, a, tl, pl = psc.tree_lists(tree)
    assert tree.info.nodes == len(wa) == len(a)
    assert pc.same_f32(box, wbox)
    mn, mx = upc.root_rule(ms.pos, ms.moved_probes)
    assert np.array_equal(uc.bits(np.concatenate(tree.root_box)), uc.bits(np.concatenate([mn, mx])))
    leaf = (wa & LEAF) != 0
    assert np.array_equal((a & LEAF) != 0, leaf)
    assert np.array_equal(a[~leaf], wa[~leaf])
    assert np.array_equal(a[leaf] & ~LEAF, [len(t) for t, lf in zip(wtris, leaf) if lf])
    for i in range(len(a)):
        assert np.array_equal(tl[i], wtris[i]), i
        assert np.array_equal(pl[i], wprs[i]), i
    assert tree.probe_info() == (7, 9, 14)
