#!/usr/bin/env python3
"""Several lights in one light map: vrt_lightmap_build_lights against what a
caller could do before it.

On the sponza-proxy at detail 1.0, depth 6, with four lights -- the
reference's light pose (VRT/main.cc:80-83) and three camera-sweep poses lifted
above the atrium and looking down into it -- each with a 1024 x 1024 film, in
one process, after a warm-up, alternating, the median of --reps repetitions
(at least 7), a host clock around calls that end in a synchronise:
  (a) four consecutive vrt_lightmap_build calls, one per light (each replaces
      the map of the one before: the same work, not the same result);
  (b) one vrt_lightmap_build_lights with the four;
  (c) vrt_lightmap_build of the first light at 2048 x 1024 twice over: the
      same sample count as (b) through the one-light kernels.
The spread is each case's max - min over the repetitions.

  --only X   run case X alone (for a profiler run of its own: with
             rocprofv3 --kernel-trace --stats around `--only b` the kernel
             times of k_light_lights and its tail are read from the stats)
Prints and, with --out, writes one JSON document."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

try:  # torch first: one HIP runtime per process
    import torch  # noqa: F401
except Exception:
    torch = None

import voxelraytrace20190722_amd as vrt  # noqa: E402

UP = (0.0, 1.0, 0.0)


def lights_of(tree, n_film):
    mn, mx = tree.root_box
    height = float(mx[1] - mn[1])
    centre = tuple(float(0.5 * (a + b)) for a, b in zip(mn, mx))
    cams = [vrt.Camera(vrt.to_radian(60), (1.0, 10.0, 1.0), (0.0, 0.0, 0.0), UP)]
    for i in (2, 7, 12):
        fov, eye, spot, up = vrt.sweep_pose(mn, mx, i, 16)
        eye = (float(eye[0]), float(mx[1] + 0.75 * height), float(eye[2]))
        cams.append(vrt.Camera(fov, eye, (centre[0], float(mn[1]), centre[2]), UP))
    colours = [(1.0, 1.0, 1.0), (1.0, 0.8, 0.6), (0.4, 0.6, 1.0), (0.9, 0.2, 0.3)]
    film = vrt.Film(1, 1, n_film, n_film)
    return [vrt.Light(c, film, col) for c, col in zip(cams, colours)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--film", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=["a", "b", "c"])
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.reps < 7 and not args.only:
        ap.error("--reps must be at least 7")
    tree = vrt.VoxelOctree(vrt.SceneData.proxy(args.detail, 1), args.depth)
    lights = lights_of(tree, args.film)
    wide = vrt.Film(1, 1, 2 * args.film, args.film)
    hits = {}

    def case_a():
        hits["a"] = [tree.lightmap(l.camera, l.film) for l in lights]

    def case_b():
        hits["b"] = tree.lightmap_lights(lights)

    def case_c():
        hits["c"] = [tree.lightmap(lights[0].camera, wide) for _ in range(2)]

    cases = {"a": case_a, "b": case_b, "c": case_c}
    names = [args.only] if args.only else ["a", "b", "c"]
    for _ in range(args.warmup):
        for k in names:
            cases[k]()
    ms = {k: [] for k in names}
    for _ in range(args.reps):
        for k in names:
            t0 = time.perf_counter()
            cases[k]()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    out = {"scene": f"proxy detail {args.detail}", "depth": args.depth, "film": [args.film, args.film],
           "lights": len(lights), "reps": args.reps, "hits": hits, "stats_last": tree.lightmap_stats(),
           "scratch_bytes": tree.scratch_bytes()[0]}
    for k in names:
        out[k] = {"median_ms": statistics.median(ms[k]), "min_ms": min(ms[k]), "max_ms": max(ms[k]),
                  "spread_ms": max(ms[k]) - min(ms[k]), "all_ms": [round(v, 4) for v in ms[k]]}
    if "a" in out and "b" in out:
        out["b_over_a"] = out["b"]["median_ms"] / out["a"]["median_ms"]
        assert sum(hits["a"]) == hits["b"], (hits["a"], hits["b"])
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
