"""The beam entry (k_unit_entry in vrt_kernels.hip) on the
CPU: a numpy float32 restatement of the pre-pass (tests/beam_entry_cases.py)
against a per-ray restatement of ray_march's finite-slab walk.  For every unit
with a record, each of its 64 rays walked alone through the committed
iterations -- its own slab tests, its own triangle-box skips, the chain order
where it passes the criterion and the oracle's sort8 elsewhere -- must stand
at exactly the recorded loop-top state."""
import numpy as np
import pytest

import pyoracle as po
import voxelraytrace20190722_amd as vrt
import beam_entry_cases as bc

DETAIL = 0.02  # the coarse proxy (48-B leaf records, the persistent render's format, from depth 6 on)
POSES = (0, 5, 11)


@pytest.fixture(scope="module", params=[4, 5, 6], ids=lambda d: "depth%d" % d)
def scene(request):
    sd = vrt.SceneData.proxy(DETAIL, 1)
    vo = vrt.VoxelOctree(sd, request.param, device=-1)
    return vo, bc.Tree(vo, sd)


def _check_unit(tree, o, d):
    """-> (stop reason, committed expansions); asserts the per-ray states."""
    rec, iters, nexp, why = bc.prepass(tree, o, d)
    if rec[0] == bc.ENTRY_NONE:
        return why, 0
    want = bc.record_entries(rec)
    assert all(y >> 24 > 0 for _, y in want) and len(want) <= bc.ENTRY_MAX
    got = bc.walk_rays(po, tree, o, d, iters)
    for lane, g in enumerate(got):
        assert g == want, (why, iters, lane, g, want)
    return why, nexp


def test_sweep_frames(scene):
    """Every unit of three 64x64 sweep frames."""
    vo, tree = scene
    mn, mx = vo.root_box
    film = vrt.Film(1, 1, 64, 64)
    beyond = total = 0
    for pose in POSES:
        cam = vrt.Camera(*vrt.sweep_pose(mn, mx, pose, 16))
        o, d = bc.frame_units(cam, film)
        res = [_check_unit(tree, o, d[u]) for u in range(d.shape[0])]
        nexp = np.array([n for _, n in res])
        why = [w for w, _ in res]
        print(f"pose {pose}: {len(res)} units, committed expansions mean {nexp.mean():.2f}, "
              f"stops { {w: why.count(w) for w in sorted(set(why))} }")
        # not vacuous: most units commit the root's expansion ...
        assert (nexp >= 1).sum() > 0.5 * len(res)
        beyond += int((nexp >= 2).sum())
        total += len(res)
    # ... and, a unit of a 64x64 frame being 1/16 of the view wide, still more
    # than a third go on past it (a pre-pass that stopped at the root: none)
    assert beyond > total / 3


def test_adversarial_units(scene):
    """Units about node mid-planes, edges and corners, an eye on a split
    plane, a sign change inside the unit, near-axis units, eyes outside the
    root box and beyond lb_reach."""
    vo, tree = scene
    units = bc.adversarial_units(tree)
    seen = {}
    for name, o, d in units:
        why, nexp = _check_unit(tree, o, d)
        seen.setdefault(name, []).append((why, nexp))
    for name, r in seen.items():
        why = [w for w, _ in r]
        print(f"{name}: {len(r)} units, stops { {w: why.count(w) for w in sorted(set(why))} }")
    assert set(seen) == {"feature", "near_axis", "sign", "on_plane", "outside", "far"}
    every = [w for r in seen.values() for w, _ in r]
    # "no entry" records occur, and so do units with committed work
    assert any(w == "signs" for w, _ in seen["sign"])
    assert sum(w in ("signs", "root", "root expansion", "not fast") for w in every) >= 5
    assert sum(n >= 1 for r in seen.values() for _, n in r) >= len(every) // 3
    # a far eye disables the triangle-box skip, a near-axis unit the chain order
    assert not tree.lbok(units[-1][1])
    nochain = [not (bc.prepass(tree, o, d)[0][0] & bc.CHAIN_BIT) for name, o, d in units if name == "near_axis"]
    print(f"near_axis: {sum(nochain)} of {len(nochain)} units fail the criterion")
    assert sum(nochain) >= 1 and any(w in ("order", "root expansion") for w, _ in seen["near_axis"])


def test_root_miss(scene):
    vo, tree = scene
    # a unit that looks away from the scene from outside it: not certainly hit
    mn, mx = vo.root_box
    cen = (mn.astype(np.float64) + mx) * .5
    eye = cen + 3.0 * (mx - mn)
    c, r, u = bc._frame_of(eye - cen)
    rec, _, _, why = bc.prepass(tree, np.float32(eye), bc.bundle(eye, c, r, u, 0.01))
    assert rec[0] == bc.ENTRY_NONE and why == "root"
