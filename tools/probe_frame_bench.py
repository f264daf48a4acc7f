#!/usr/bin/env python3
"""Timing of a probe scene's view frame shaded on the device
(vrt_render_trace_probes_device) against the only way to the same frame before
it: vrt_trace_batch_device over the view's prepared rays with parts.hits, the
hits and colours copied to the host, vrt_probe_shade_hits there, and the film
sum -- run through --parent LIB, a build of the parent commit (without it: the
package's library, which still has that path).

Workload as tools/probe_scene_bench.py: the bench's sponza-proxy at --depth
with the light map of the driver's light camera (VRT/main.cc:75-78), the
driver's own 100 probes (VRT/main.cc:56-61) as voxels with gathered SGs, and
the --film^2 view (VRT/main.cc:112-123).  Both paths end with the frame in host
memory.  The device call is timed by HIP events (the render alone) and by wall
clock (render + image copy); the yardstick by wall clock (it has host work in
the middle) with its device part by events.  Windows alternate inside every
round; median and spread of the rounds.  The two frames are compared bit for
bit (NaN matching NaN) before anything is timed.

--once N runs the device call N times without timing (for a kernel trace by a
profiler around this script: k_trace_prim_mixed, then k_cones_film<true>).

usage: tools/probe_frame_bench.py [--depth 6] [--film 1024] [--rounds 5] [--parent LIB] [--out DIR]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

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
    ap.add_argument("--reps", type=int, default=3, help="frames per timed window")
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--light-n", type=int, default=2048)
    ap.add_argument("--parent", default=None, help="a libvrt.so of the parent commit for the yardstick")
    ap.add_argument("--once", type=int, default=0, help="run the device call this many times, no timing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_frame"))
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
    sgs = tree.gather_probes(res, (1.0, 1.0, 1.0))
    cam, film = vrt.Camera(*VIEW), vrt.Film(1, 1, a.film, a.film)
    nx = ny = a.film
    st = torch.cuda.current_stream().cuda_stream

    # the device call: the frame on the device, then in pinned host memory
    d_img = torch.zeros((ny, nx, 3), device="cuda")
    h_img = torch.zeros((ny, nx, 3)).pin_memory()

    def device_frame():
        tree.render_trace_probes_device(cam, film, 0, 1, 1, d_img.data_ptr(), res, st)

    def device_frame_to_host():
        device_frame()
        h_img.copy_(d_img, non_blocking=True)
        torch.cuda.synchronize()

    if a.once:
        for _ in range(a.once):
            device_frame()
        torch.cuda.synchronize()
        print(json.dumps({"once": a.once, "build_id": vrt.build_id()}))
        return

    # the yardstick: the same probe scene in the parent's library
    ph = C.c_void_p()
    pr = np.ascontiguousarray(probes)
    ok(P, P.vrt_scene_create_probes(C.byref(desc), pr.ctypes.data_as(C.POINTER(_ffi.Probe)), len(pr), a.depth, 0, 0,
                                    C.byref(ph)), "vrt_scene_create_probes (yardstick)")
    ok(P, P.vrt_lightmap_build(ph, C.byref(lcam.c), C.byref(lfilm.c), None), "vrt_lightmap_build (yardstick)")
    rec = np.ascontiguousarray(np.concatenate([sgs["a"], sgs["d"], sgs["s"][:, :, None]], axis=2))
    ok(P, P.vrt_scene_set_probe_sgs(ph, rec.ctypes.data_as(C.POINTER(_ffi.SGRec))), "vrt_scene_set_probe_sgs")
    rays = np.concatenate([cam.gen_rays4(film, px, py) for py in range(ny) for px in range(nx)])
    n = len(rays)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
    d_rgb = torch.zeros((n, 3), device="cuda")
    d_hits = torch.zeros((n, 9), dtype=torch.int32, device="cuda")
    h_rgb = torch.zeros((n, 3)).pin_memory()
    h_hits = torch.zeros((n, 9), dtype=torch.int32).pin_memory()
    parts = _ffi.TraceParts(d_hits.data_ptr(), None, None, None)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    y_dev_ms = []

    def yardstick():
        ev[0].record()
        ok(P, P.vrt_trace_batch_device(ph, d_rays.data_ptr(), n, res, d_rgb.data_ptr(), C.byref(parts), st),
           "vrt_trace_batch_device (yardstick)")
        ev[1].record()
        h_hits.copy_(d_hits, non_blocking=True)
        h_rgb.copy_(d_rgb, non_blocking=True)
        torch.cuda.synchronize()
        y_dev_ms.append(ev[0].elapsed_time(ev[1]))
        rgb = h_rgb.numpy()
        ok(P, P.vrt_probe_shade_hits(ph, C.c_void_p(h_hits.data_ptr()), n, rgb.ctypes.data_as(_ffi.f32p), None),
           "vrt_probe_shade_hits (yardstick)")
        c = rgb.reshape(ny, nx, 4, 3)  # Film::add(c * .25f) in sample order from zero
        acc = np.zeros((ny, nx, 3), f32)
        for j in range(4):
            acc = acc + c[:, :, j, :] * f32(.25)
        return acc

    device_frame_to_host()
    want = yardstick()
    got = h_img.numpy()
    same = bool(np.all((np.isnan(got) & np.isnan(want)) | (got.view(np.uint32) == want.view(np.uint32))))
    on_probe = float((h_hits.numpy()[:, 1] >= sd.ntri).mean())

    def wall(fn, reps):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t0) * 1e3 / reps

    def events(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    device_frame_to_host()
    ms = {"device_call_events": [], "device_call_to_host_wall": [], "yardstick_to_host_wall": [],
          "yardstick_device_part_events": []}
    for _ in range(a.rounds):
        y_dev_ms.clear()
        ms["yardstick_to_host_wall"].append(wall(yardstick, a.reps))
        ms["yardstick_device_part_events"].append(float(np.mean(y_dev_ms)))
        ms["device_call_events"].append(events(device_frame, a.reps))
        ms["device_call_to_host_wall"].append(wall(device_frame_to_host, a.reps))

    def summary(v):
        med = float(np.median(v))
        return {"ms_median": med, "ms_rounds": [float(x) for x in v], "spread": float((max(v) - min(v)) / med)}

    t = {k: summary(v) for k, v in ms.items()}
    doc = {"workload": {"detail": a.detail, "depth": a.depth, "film": a.film, "samples": n, "light_n": a.light_n,
                        "probes": len(probes), "nodes": int(tree.info.nodes), "rounds": a.rounds,
                        "frames_per_window": a.reps, "device": torch.cuda.get_device_name(0),
                        "build_id": vrt.build_id(), "yardstick_library": a.parent or "package",
                        "expf_flavour": vrt.expf_flavour()},
           "probe_share": on_probe, "frames_bit_equal": same, "times": t,
           "yardstick_over_device_call_to_host": t["yardstick_to_host_wall"]["ms_median"]
           / t["device_call_to_host_wall"]["ms_median"]}
    P.vrt_scene_destroy(ph)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "probe_frame_bench.json"), "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
