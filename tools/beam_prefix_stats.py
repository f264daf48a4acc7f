#!/usr/bin/env python3
"""How much of a unit's walk the beam entry commits, on the
host: the numpy restatement of k_unit_entry (tests/beam_entry_cases.py, with
the triangle-box skip) over sampled 4x4-pixel units -- and, for comparison,
8x8-pixel tiles -- of sweep poses.  Prints one JSON object: committed
expansions and iterations, stack entries at the stop, stop reasons.

usage: tools/beam_prefix_stats.py [--width 1920 --height 1080 --depth 8] [--units 40] [--poses 0,2,...]
                                  [--out profiles/beam_entry/prefix_stats.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import voxelraytrace20190722_amd as vrt  # noqa: E402
import beam_entry_cases as bc  # noqa: E402


def unit_dirs(cam, film, tx, ty, quad):
    """The 64 directions of a unit (quad 0..3), or the 256 of its tile (quad None)."""
    x0, y0, n = (tx * 8, ty * 8, 8) if quad is None else (tx * 8 + (quad & 1) * 4, ty * 8 + (quad >> 1) * 4, 4)
    r = np.stack([cam.gen_rays4(film, x0 + i % n, y0 + i // n) for i in range(n * n)])
    return r[0, 0, 0:3].copy(), r[:, :, 3:6].reshape(-1, 3)


def summarise(rows):
    why = [w for _, _, _, w in rows]
    out = {"units": len(rows), "stops": {w: why.count(w) for w in sorted(set(why))}}
    for name, col in (("expansions", 2), ("iterations", 1), ("entries", 0)):
        v = np.array([r[col] for r in rows], float)
        out[name] = {"mean": round(float(v.mean()), 2), "p10": float(np.percentile(v, 10)),
                     "p50": float(np.percentile(v, 50)), "p90": float(np.percentile(v, 90))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--units", type=int, default=40, help="sampled units (and tiles) per pose")
    ap.add_argument("--poses", default="0,2,4,6,8,10,12,14")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sd = vrt.SceneData.proxy(a.detail, 1)
    vo = vrt.VoxelOctree(sd, a.depth, device=-1)
    tree = bc.Tree(vo, sd)
    mn, mx = vo.root_box
    film = vrt.Film(1, 1, a.width, a.height)
    rng = np.random.default_rng(a.seed)
    units, tiles = [], []
    for pose in [int(x) for x in a.poses.split(",")]:
        cam = vrt.Camera(*vrt.sweep_pose(mn, mx, pose, 16))
        for _ in range(a.units):
            tx, ty, q = int(rng.integers(0, a.width // 8)), int(rng.integers(0, a.height // 8)), int(rng.integers(0, 4))
            for rows, quad in ((units, q), (tiles, None)):
                o, d = unit_dirs(cam, film, tx, ty, quad)
                rec, iters, nexp, why = bc.prepass(tree, o, d)
                n = 0 if rec[0] == bc.ENTRY_NONE else int(rec[0]) & 0xFF
                rows.append((n, iters, nexp, why))
    res = {"width": a.width, "height": a.height, "depth": a.depth, "detail": a.detail, "poses": a.poses,
           "unit_4x4": summarise(units), "tile_8x8": summarise(tiles)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
