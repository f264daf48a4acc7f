#!/usr/bin/env python3
"""Where the beam pre-pass runs, from a rocprofv3 `--kernel-trace` CSV of a
run with frames in flight: per frame (one k_unit_entry dispatch, the last
--frames of the trace),

  gap_us       k_unit_entry's start after the end of the render that finished
               last before it (small: it started in that render's tail)
  entry_us     how long k_unit_entry ran
  to_render_us its own render's start (the next k_render_p on the same queue)
               after k_unit_entry's end
  renders      k_render_p dispatches running at k_unit_entry's start / at its
               end / at any time during it

and the averages of both kernels' durations over those frames.

usage: tools/prepass_timeline.py KERNEL_TRACE_CSV OUT_JSON [--frames 32]
"""
import argparse
import csv
import json
import statistics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("out")
    ap.add_argument("--frames", type=int, default=32)
    a = ap.parse_args()
    rows = [(x["Kernel_Name"], int(x["Queue_Id"]), int(x["Start_Timestamp"]), int(x["End_Timestamp"]))
            for x in csv.DictReader(open(a.csv))]
    rows.sort(key=lambda r: r[2])
    ent = [r for r in rows if "k_unit_entry" in r[0]]
    ren = [r for r in rows if "k_render_p" in r[0]]
    frames = []
    for _, q, s, e in ent[-a.frames:]:
        before = [r[3] for r in ren if r[3] <= s]
        own = [r for r in ren if r[1] == q and r[2] >= e]
        frames.append({
            "gap_us": round((s - max(before)) / 1e3, 1) if before else None,
            "entry_us": round((e - s) / 1e3, 1),
            "to_render_us": round((own[0][2] - e) / 1e3, 1) if own else None,
            "render_us": round((own[0][3] - own[0][2]) / 1e3, 1) if own else None,
            "renders_at_start": sum(1 for r in ren if r[2] <= s < r[3]),
            "renders_at_end": sum(1 for r in ren if r[2] <= e < r[3]),
            "renders_during": sum(1 for r in ren if r[2] < e and r[3] > s),
        })
    mean = lambda k: round(statistics.mean(f[k] for f in frames if f[k] is not None), 1)  # noqa: E731
    span = ent[-1][2] - ent[-len(frames)][2]
    out = {"frames": frames,
           "mean": {k: mean(k) for k in ("gap_us", "entry_us", "to_render_us", "render_us", "renders_at_start",
                                         "renders_at_end", "renders_during")},
           "entry_to_entry_us": round(span / 1e3 / max(1, len(frames) - 1), 1)}
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out["mean"]), "entry to entry", out["entry_to_entry_us"], "us")


if __name__ == "__main__":
    main()
