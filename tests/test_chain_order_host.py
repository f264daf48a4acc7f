"""The chain order against the reference's sort, on the CPU: a
numpy float32 restatement of expand_v2<2> (tests/chain_order_cases.py) gives
each case's hit mask and travorder keys, the oracle's sort8 (libstdc++
std::sort, as the reference) orders them, and wherever the per-ray criterion
passes and the hit children form a chain the order by octant alone must be
that order."""
import numpy as np
import pytest

import pyoracle as po
import chain_order_cases as cc


@pytest.fixture(scope="module")
def wmin():
    return cc.scene_spacing()


def _check(fam, wmin):
    """-> (cases with >= 2 hit children, of those: criterion and chain, of
    those: order differs from the reference)."""
    ev = cc.evaluate(fam, wmin)
    # (a diagonal through the centre touches all 8 children: never a chain)
    assert not np.any(ev["chain"] & (ev["cnt"] > 4))
    multi = ev["cnt"] >= 2
    use = multi & ev["crit"] & ev["chain"]
    idx = np.nonzero(use)[0]
    ref = cc.reference_order(po, ev["hm"][idx], ev["dist"][idx])
    bad = np.any(ref != ev["order"][idx], axis=1)
    return int(multi.sum()), int(use.sum()), int(bad.sum()), ev


def test_chain_tables_match_the_bit_forms():
    """chain_order2 / chain_order4's bit arithmetic, restated, against the
    definition (pairwise comparable; order by far-side axes) for every (s, hm)."""
    for s in range(8):
        for hm in range(256):
            hc = 0
            for ci in range(8):
                if (hm >> ci) & 1:
                    hc |= 1 << (ci ^ s)
            l1, l2 = hc & 0x16, hc & 0x68
            rev = int(f"{hc:08b}"[::-1], 2)
            valid4 = not ((l1 & (l1 - 1)) | (l2 & (l2 - 1)) | (hc & rev & 0x16))
            assert valid4 == bool(cc.CHAIN_VALID[s, hm]), (s, hm)
            kids = [ci for ci in range(8) if (hm >> ci) & 1]
            if valid4:
                order4 = [c ^ s for c in range(8) if (hc >> c) & 1]
                assert order4 == [int(x) for x in cc.CHAIN_ORDER[s, hm] if x >= 0], (s, hm)
            if len(kids) == 2:
                i0, i1 = kids
                x = i0 ^ i1
                a = (i0 ^ s) & x
                assert (a == 0 or a == x) == bool(cc.CHAIN_VALID[s, hm]), (s, hm)
                if a == 0 or a == x:
                    want = [i1, i0] if a == x else [i0, i1]
                    assert want == [int(v) for v in cc.CHAIN_ORDER[s, hm, :2]], (s, hm)


def test_random_rays(wmin):
    """>= 100 k rays aimed into or around the node from an origin inside the
    scene: no mismatch, and the chain order applies to >= 90 % of the cases
    that order anything."""
    multi, use, bad, _ = _check(cc.family_random(1, 120_000), wmin)
    print(f"random: {multi} cases with >= 2 hit children, {use} pass ({100.0 * use / multi:.3f} %), {bad} mismatches")
    assert bad == 0
    assert multi >= 50_000 and use >= 0.90 * multi


def test_near_axis_rays(wmin):
    """One direction component scaled by 1e-3 .. 1e-8: >= 25 % of the cases
    with >= 2 hit children fail the criterion (the fallback), no mismatch
    among those that pass."""
    multi, use, bad, ev = _check(cc.family_near_axis(2, 60_000), wmin)
    fail = int(((ev["cnt"] >= 2) & ~ev["crit"]).sum())
    print(f"near-axis: {multi} cases, {fail} fail the criterion ({100.0 * fail / multi:.2f} %), "
          f"{use} pass and chain, {bad} mismatches")
    assert bad == 0
    assert fail >= 0.25 * multi
    assert use > 0


@pytest.mark.parametrize("family", ["diagonal", "features"])
def test_degenerate_directions_and_targets(wmin, family):
    """Exactly diagonal directions (|dx| = |dy|, |dx| = |dy| = |dz|), and rays
    at box corners, edges and mid-plane crossings: no mismatch where the
    criterion passes and the set is a chain."""
    fam = cc.family_diagonal(3, 40_000) if family == "diagonal" else cc.family_features(4, 40_000)
    if family == "diagonal":
        d = np.abs(fam[3])
        srt = np.sort(d, 1)
        assert np.all((srt[:, 0] == srt[:, 1]) | (srt[:, 1] == srt[:, 2]))
    multi, use, bad, ev = _check(fam, wmin)
    nonchain = int(((ev["cnt"] >= 2) & ~ev["chain"]).sum())
    print(f"{family}: {multi} cases, {use} pass and chain, {nonchain} non-chain sets, {bad} mismatches")
    assert bad == 0
    assert use > 1000


def test_far_origin_rejects(wmin):
    """An origin 100 extents away: R_k makes the rounding bound larger than
    the near-axis gaps, so the criterion rejects every ray -- while the same
    directions from a point of the ray near the scene mostly pass."""
    fam = cc.family_far(5, 20_000)
    ev = cc.evaluate(fam, wmin)
    assert not np.any(ev["crit"])
    bmin, bmax, o, d = fam
    ext = float(np.max(cc.ROOT_MAX - cc.ROOT_MIN))
    near = (o.astype(np.float64) + d.astype(np.float64) * 99.0 * ext).astype(np.float32)
    ev2 = cc.evaluate((bmin, bmax, near, d), wmin)
    print(f"far origin: 0 of {len(d)} pass; from 1 extent: {int(ev2['crit'].sum())}")
    assert ev2["crit"].mean() > 0.5
    multi, use, bad, _ = _check((bmin, bmax, near, d), wmin)
    assert bad == 0
