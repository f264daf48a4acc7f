#!/usr/bin/env python3
"""Timing of trace() on a scene with light probes as voxels
(vrt_scene_create_probes + vrt_trace_batch_device, the mixed even_invisible
march) against the same call on the triangle-only scene.

Workload: the bench's sponza-proxy at --depth with the light map of the
driver's light camera (VRT/main.cc:75-78), the reference driver's own 100
probes (VRT/main.cc:56-61) as voxels, and the --film^2 view's gen_rays4 rays
(VRT/main.cc:112-123) prepared once on the device.  Yardstick: the same rays
through vrt_trace_batch_device on the triangle-only scene, by --parent LIB (a
build of the parent commit) or, without it, by the package's library.  Device
calls, HIP events on the stream after a warm-up, windows of >= --window
seconds, the two paths alternating inside every round; median and spread of
the rounds.  Also reported: the share of rays that end on a probe, and that
the rays ending on triangles in both scenes get the same colour.

--once N runs each path N times without timing (for a kernel trace by a
profiler around this script: the mixed march is k_trace_batch_prim_mixed, the
triangle-only one k_trace_batch_prim).

usage: tools/probe_scene_bench.py [--depth 6] [--film 1024] [--rounds 5] [--parent LIB] [--out DIR]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import torch  # one HIP runtime: torch's

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import voxelraytrace20190722_amd as vrt  # noqa: E402
from voxelraytrace20190722_amd import _ffi  # noqa: E402

LIGHT = (vrt.to_radian(60), (1, 10, 1), (0, 0, 0), (0, 1, 0))  # VRT/main.cc:75-78
VIEW = (vrt.to_radian(90), (1.0, 1.3, -0.2), (0.0, 0.4, 0.0), (0.0, 1.0, 0.0))  # VRT/main.cc:112-115
f32 = np.float32


def load(path):
    L = C.CDLL(os.path.abspath(path))
    for name, (res, args) in _ffi.SIGNATURES.items():
        if hasattr(L, name):
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
    return L


def ok(L, rc, where):
    if rc != 0:
        raise RuntimeError(f"{where}: {rc} {L.vrt_last_error().decode(errors='replace')}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--film", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--light-n", type=int, default=2048)
    ap.add_argument("--parent", default=None, help="a libvrt.so of the parent commit for the triangle-only scene")
    ap.add_argument("--once", type=int, default=0, help="run each path this many times, no timing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_scene"))
    a = ap.parse_args()

    L = vrt.lib()
    P = load(a.parent) if a.parent else L
    sd = vrt.SceneData.proxy(a.detail, 1)
    desc = sd.desc()
    lcam, lfilm = vrt.Camera(*LIGHT), vrt.Film(1, 1, a.light_n, a.light_n)
    rp = vrt.probe_points(0xc01dbeefdeadbead, 100)  # VRT/main.cc:57-61
    probes = np.ascontiguousarray(np.concatenate([rp + np.array((0.5, 0.4, 0.0), f32), np.full((100, 1), 0.1, f32)],
                                                 axis=1).astype(f32))
    tree = vrt.VoxelOctree(sd, a.depth, device=0, probes=probes)
    tree.lightmap(lcam, lfilm)
    res = tree.min_voxel(a.depth)
    tree.gather_probes(res, (1.0, 1.0, 1.0))
    ph = C.c_void_p()
    ok(P, P.vrt_scene_create(C.byref(desc), a.depth, 0, C.byref(ph)), "vrt_scene_create (yardstick)")
    ok(P, P.vrt_lightmap_build(ph, C.byref(lcam.c), C.byref(lfilm.c), None), "vrt_lightmap_build (yardstick)")

    cam, film = vrt.Camera(*VIEW), vrt.Film(1, 1, a.film, a.film)
    rays = np.concatenate([cam.gen_rays4(film, px, py) for py in range(a.film) for px in range(a.film)])
    n = len(rays)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
    d_rgb = [torch.zeros((n, 3), device="cuda") for _ in range(2)]
    d_hits = [torch.zeros((n, 9), dtype=torch.int32, device="cuda") for _ in range(2)]
    parts = [_ffi.TraceParts(h.data_ptr(), None, None, None) for h in d_hits]
    st = torch.cuda.current_stream().cuda_stream

    def probe_scene(with_hits=False):
        ok(L, L.vrt_trace_batch_device(tree.h, d_rays.data_ptr(), n, res, d_rgb[0].data_ptr(),
                                       C.byref(parts[0]) if with_hits else None, st), "vrt_trace_batch_device")

    def yardstick(with_hits=False):
        ok(P, P.vrt_trace_batch_device(ph, d_rays.data_ptr(), n, res, d_rgb[1].data_ptr(),
                                       C.byref(parts[1]) if with_hits else None, st),
           "vrt_trace_batch_device (yardstick)")

    probe_scene(True)
    yardstick(True)
    torch.cuda.synchronize()
    on_probe = d_hits[0][:, 1] >= sd.ntri
    same_tri = (~on_probe) & (d_hits[0][:, 1] == d_hits[1][:, 1]) & (d_hits[0][:, 3:6] == d_hits[1][:, 3:6]).all(dim=1)
    # context only: some of the driver's probes lie outside the triangles' box, so the probe
    # scene's root box, voxels and light map are not the triangle-only scene's
    same_rgb = float((d_rgb[0][same_tri].view(torch.int32) == d_rgb[1][same_tri].view(torch.int32)).all(dim=1)
                     .float().mean())
    doc = {"workload": {"detail": a.detail, "depth": a.depth, "film": a.film, "rays": n, "light_n": a.light_n,
                        "probes": len(probes), "probe_info": tree.probe_info(), "nodes": int(tree.info.nodes),
                        "rounds": a.rounds, "window_s": a.window, "device": torch.cuda.get_device_name(0),
                        "build_id": vrt.build_id(), "yardstick_library": a.parent or "package"},
           "probe_share": float(on_probe.float().mean()),
           "same_triangle_share": float(same_tri.float().mean()), "same_triangle_same_rgb_share": same_rgb}
    if a.once:
        for _ in range(a.once):
            probe_scene()
            yardstick()
        torch.cuda.synchronize()
        print(json.dumps(doc))
        return

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    items = [("triangle_only", yardstick), ("probe_scene", probe_scene)]
    reps = {}
    for name, fn in items:
        window(fn, 2)
        reps[name] = max(3, math.ceil(a.window * 1000.0 / window(fn, 3)))
    ms = {name: [] for name, _ in items}
    for _ in range(a.rounds):
        for name, fn in items:
            ms[name].append(window(fn, reps[name]))

    def summary(v):
        med = float(np.median(v))
        return {"ms_median": med, "ms_rounds": [float(x) for x in v], "spread": float((max(v) - min(v)) / med)}

    t = {name: summary(v) for name, v in ms.items()}
    doc.update({"calls_per_window": reps, "times": t,
                "probe_scene_over_triangle_only": t["probe_scene"]["ms_median"] / t["triangle_only"]["ms_median"],
                "mrays_per_s": {k: n / v["ms_median"] / 1e3 for k, v in t.items()}})
    P.vrt_scene_destroy(ph)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "probe_scene_bench.json"), "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
