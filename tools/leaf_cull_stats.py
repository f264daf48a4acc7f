#!/usr/bin/env python3
"""Where a primary frame's leaf-record tests go, and how many of them a
per-record triangle box would cull -- host only (the oracle's walk, no GPU),
so a scene or depth can be judged before any kernel work.

Per sampled work unit of the primary render (a 4x4-pixel quadrant x 4
gen_rays4 samples = one wave, one ray per lane) it takes the leaf that ends
each lane's walk (the hit leaf) and counts, per lane, that leaf's records and
the records whose eps-enlarged triangle box (march_nodes' box of a
one-triangle leaf, eps = 2^-16 x the scene extent) the ray's line meets in
the kernel's fp32 test (line_meets_box, restated op for op).  A wave runs the
union of its lanes' loops, so the per-unit figures are maxima over the lanes.
The reference's own counters give the other side of the split: triangle
tests in leaves that end no walk (T minus the final leaf's records).

usage: tools/leaf_cull_stats.py [--depth 8] [--detail 1.0] [--seed 1]
           [--width 1920 --height 1080] [--poses 0,5,9,13] [--units 558]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyoracle as po  # noqa: E402
import voxelraytrace20190722_amd as vrt  # noqa: E402

F = np.float32


def enlarged_boxes(pos, ext):
    """march_nodes' box of each triangle (n, 9) alone: +- 2^-16 * ext, rounded
    outward to float -> (n, 3) lo, (n, 3) hi."""
    eps = np.ldexp(float(ext), -16)
    p = pos.reshape(-1, 3, 3).astype(np.float64)
    lo, hi = p.min(1) - eps, p.max(1) + eps
    flo, fhi = lo.astype(F), hi.astype(F)
    flo = np.where(flo.astype(np.float64) > lo, np.nextafter(flo, F(-np.inf)), flo)
    fhi = np.where(fhi.astype(np.float64) < hi, np.nextafter(fhi, F(np.inf)), fhi)
    return flo, fhi


def line_meets_boxes(lo, hi, o, dinv):
    """line_meets_box() in fp32, op for op, one ray against (n, 3) boxes."""
    a = (lo - o) * dinv
    b = (hi - o) * dinv
    t0 = np.minimum(a, b).max(1)
    t1 = np.maximum(a, b).min(1)
    return t0 <= t1


def pct(v, q):
    return float(np.percentile(v, q)) if len(v) else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--poses", default="0,5,9,13", help="poses of the 16-pose sweep")
    ap.add_argument("--units", type=int, default=558, help="sampled units over all poses")
    ap.add_argument("--heavy", type=int, default=16, help="a unit is heavy from this many loop iterations")
    ap.add_argument("--rng", type=int, default=20261019)
    a = ap.parse_args()

    sd = vrt.SceneData.proxy(a.detail, a.seed)
    sc = po.Scene(sd, a.depth)
    info, box = sc.info()
    ext = float(np.max(box[3:6] - box[0:3]))
    vox, cnt, tris = sc.leaves()
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
    order = np.argsort(vox, kind="stable")
    svox = vox[order]
    lo, hi = enlarged_boxes(np.asarray(sd.pos, F).reshape(-1, 9), ext)

    out = {"scene": {"detail": a.detail, "seed": a.seed, "depth": a.depth, "nonempty_leaves": int(len(cnt)),
                     "refs": int(cnt.sum())},
           "records_per_leaf": {"mean": round(float(cnt.mean()), 2), "p50": pct(cnt, 50), "p90": pct(cnt, 90),
                                "p99": pct(cnt, 99), "max": int(cnt.max())}}

    poses = [int(x) for x in a.poses.split(",")]
    rng = np.random.default_rng(a.rng)
    lane_n, lane_s, lane_T = [], [], []      # per hit lane: final leaf's records, box survivors, reference T
    unit_n, unit_s, unit_T = [], [], []      # per unit: maxima over its lanes
    per_pose = max(1, a.units // len(poses))
    left = a.units
    for pi, pose in enumerate(poses):
        nu = left if pi == len(poses) - 1 else per_pose
        left -= nu
        fov, eye, spot, up = vrt.sweep_pose(box[0:3], box[3:6], pose, 16)
        cam = po.camera(fov, eye, spot, up)
        for _ in range(nu):
            ux, uy = int(rng.integers(a.width // 4)), int(rng.integers(a.height // 4))
            rays = np.concatenate([po.gen_rays4(cam, 1.0, 1.0, a.width, a.height, 4 * ux + i, 4 * uy + j)
                                   for j in range(4) for i in range(4)])
            res = sc.ray_march(rays)
            un, us, uT = 0, 0, 0
            for l in range(64):
                T = int(res["counters"][l, 2])
                uT = max(uT, T)
                if not res["hit"][l]:
                    continue
                k = order[np.searchsorted(svox, res["voxel"][l])]
                ids = tris[first[k]:first[k] + cnt[k]]
                o = rays[l, 0:3]
                dinv = (F(1) / rays[l, 3:6]).astype(F)
                with np.errstate(invalid="ignore", over="ignore"):
                    s = int(line_meets_boxes(lo[ids], hi[ids], o, dinv).sum())
                lane_n.append(len(ids))
                lane_s.append(s)
                lane_T.append(T)
                un, us = max(un, len(ids)), max(us, s)
            unit_n.append(un)
            unit_s.append(us)
            unit_T.append(uT)
    lane_n, lane_s, lane_T = (np.array(v, np.float64) for v in (lane_n, lane_s, lane_T))
    unit_n, unit_s, unit_T = (np.array(v, np.float64) for v in (unit_n, unit_s, unit_T))
    out["units"] = int(len(unit_n))
    hitting = unit_n > 0  # the per-unit figures are over units with a hit
    unit_n, unit_s, unit_T = unit_n[hitting], unit_s[hitting], unit_T[hitting]
    out["units_with_a_hit"] = int(len(unit_n))
    heavy = unit_n >= a.heavy
    out["per_lane"] = {
        "final_leaf_records": round(float(lane_n.mean()), 2),
        "box_survivors": round(float(lane_s.mean()), 2),
        "survivor_fraction": round(float(lane_s.sum() / max(1.0, lane_n.sum())), 3),
        # the reference tests every record of every leaf it enters; the
        # kernels already skip whole leaves by their union box, so this is an
        # upper bound on the tests outside the final leaf
        "reference_tests": round(float(lane_T.mean()), 2),
        "reference_tests_outside_final_leaf": round(float((lane_T - lane_n).mean()), 2),
    }
    out["per_unit_max_over_lanes"] = {
        "final_leaf_records": round(float(unit_n.mean()), 2),
        "box_survivors": round(float(unit_s.mean()), 2),
        "box_survivors_p50": pct(unit_s, 50), "box_survivors_p90": pct(unit_s, 90),
        "reference_tests": round(float(unit_T.mean()), 2),
    }
    out["heavy_units"] = {
        "threshold": a.heavy,
        "fraction_of_units": round(float(heavy.mean()), 3),
        "fraction_of_iterations": round(float(unit_n[heavy].sum() / max(1.0, unit_n.sum())), 3),
        "final_leaf_records": round(float(unit_n[heavy].mean()), 2) if heavy.any() else 0.0,
        "box_survivors": round(float(unit_s[heavy].mean()), 2) if heavy.any() else 0.0,
    }
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
