#!/usr/bin/env python3
"""Timing of the reference main() frame on the multi-device handle
(vrt_trace_frame_multi_device): light film --light-n^2, view --film^2, the
bench's sponza-proxy at --depth, as bench.py --mode trace runs it.

What is timed, in windows that alternate inside every round, each round starting
one configuration further on (median and spread of the rounds; every configuration is warmed up and compared bit for bit with
the single-scene frame before anything is timed):

  single        one vrt_trace_frame_device call per frame on one scene: the
                frame of bench.py --mode trace.  With --parent LIB (a libvrt.so
                built from the parent commit) also through that library.
  handle_1      the 1-rank handle (device_mask 1, a 1-device communicator): the
                same work plus a 1-rank gather and the unpack of the image.
                The difference to `single` is the one real measurement here.
  unpack_1      vrt_unpack_tiles_device of that image alone, by device events.
  virtual n, m  n virtual ranks (n replicas on ONE GPU, exchanges by device
                copies) in light mode m.  The ranks share one GPU, so these wall
                times rehearse the code path and say nothing about scaling; the
                exchange between devices is not measured by this tool.  The
                per-rank vrt_lightmap_stats shares are printed with them.

One JSON line per configuration, printed and written to
--out/multi_trace_bench.jsonl.

usage: tools/multi_trace_bench.py [--depth 6] [--film 1024] [--light-n 2048] [--rounds 7] [--reps 10]
                                  [--ranks 2,4,8] [--parent LIB] [--out DIR]
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

LIGHT = (vrt.to_radian(60), (1, 10, 1), (0, 0, 0), (0, 1, 0))  # VRT/main.cc:79-83
VIEW = (vrt.to_radian(90), (1.0, 1.3, -0.2), (0.0, 0.4, 0.0), (0.0, 1.0, 0.0))  # VRT/main.cc:108-112


def load(path):
    L = C.CDLL(os.path.abspath(path))
    for name, (res, args) in _ffi.SIGNATURES.items():
        if hasattr(L, name):
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
    return L


def summary(v):
    med = float(np.median(v))
    return {"ms_median": med, "ms_min": float(min(v)), "ms_max": float(max(v)),
            "spread": float((max(v) - min(v)) / med), "ms_rounds": [float(x) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--film", type=int, default=1024)
    ap.add_argument("--light-n", type=int, default=2048)
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10, help="frames per timed window")
    ap.add_argument("--ranks", default="2,4,8", help="virtual rank counts")
    ap.add_argument("--parent", default=None, help="a libvrt.so of the parent commit: its single-scene frame too")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_trace"))
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds: the median of at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool only measures on one")

    sd = vrt.SceneData.proxy(a.detail, 1)
    lcam, lfilm = vrt.Camera(*LIGHT), vrt.Film(1, 1, a.light_n, a.light_n)
    cam, film = vrt.Camera(*VIEW), vrt.Film(1, 1, a.film, a.film)
    nx = ny = a.film
    # a stream of its own: the handle takes the NULL stream as "no caller
    # stream" and returns only when the image is complete, which would keep a
    # frame's light pass from running beside the previous frame's cones
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    tree = vrt.VoxelOctree(sd, a.depth, device=0)
    res = tree.min_voxel(a.depth)
    base = {"device": torch.cuda.get_device_name(0), "build_id": vrt.build_id(), "depth": a.depth, "film": a.film,
            "light_n": a.light_n, "detail": a.detail, "rounds": a.rounds, "frames_per_window": a.reps}

    runs = {}   # name -> (frame function, image tensor)
    notes = {}  # name -> extra fields of its JSON line

    def add(name, fn, img, **extra):
        runs[name] = (fn, img)
        notes[name] = extra

    img_s = torch.zeros((ny, nx, 3), device="cuda")
    add("single", lambda: tree.trace_frame_device(lcam, lfilm, cam, film, 0, 1, 1, img_s.data_ptr(), res, sp), img_s,
        what="vrt_trace_frame_device, one scene: the frame of bench.py --mode trace")
    if a.parent:
        P = load(a.parent)
        ph, desc, hits = C.c_void_p(), sd.desc(), C.c_int64()
        rc = P.vrt_scene_create_ex(C.byref(desc), a.depth, 0, 0, C.byref(ph))
        if rc != 0:
            raise RuntimeError(f"parent vrt_scene_create_ex: {rc} {P.vrt_last_error().decode(errors='replace')}")
        img_p = torch.zeros((ny, nx, 3), device="cuda")

        def parent_frame():
            rc = P.vrt_trace_frame_device(ph, C.byref(lcam.c), C.byref(lfilm.c), C.byref(cam.c), C.byref(film.c), res,
                                          0, 1, 1, C.c_void_p(img_p.data_ptr()), C.c_void_p(sp), C.byref(hits))
            if rc != 0:
                raise RuntimeError(f"parent vrt_trace_frame_device: {rc}")
        add("single_parent", parent_frame, img_p, what="the same call through the parent commit's library",
            parent_build_id=P.vrt_build_id().decode())
    handles = []
    m1 = vrt.MultiOctree(sd, a.depth, device_mask=1)
    handles.append(m1)
    img_1 = torch.zeros((ny, nx, 3), device="cuda")
    add("handle_1", lambda: m1.trace_frame_device(lcam, lfilm, cam, film, img_1.data_ptr(), res, stream_ptr=sp), img_1,
        what="vrt_trace_frame_multi_device, 1 rank (real 1-device communicator)", ranks=1)
    virt = {}
    for n in [int(x) for x in a.ranks.split(",") if x]:
        for mode in ("replicated", "sharded"):
            m = vrt.MultiOctree(sd, a.depth, device_mask=1, virtual_ranks=n, light_mode=mode)
            handles.append(m)
            img = torch.zeros((ny, nx, 3), device="cuda")
            name = f"virtual_{n}_{mode}"
            virt[name] = m
            add(name, (lambda m=m, img=img: m.trace_frame_device(lcam, lfilm, cam, film, img.data_ptr(), res,
                                                                 stream_ptr=sp)), img,
                what="vrt_trace_frame_multi_device on virtual ranks: n replicas on ONE GPU, a rehearsal of the code "
                     "path, not a scaling result; the exchange between devices is not measured",
                ranks=n, light_mode=mode)

    # warm-up, and every configuration's frame against the single scene's, bit for bit
    for fn, _ in runs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    want = img_s.cpu().numpy().view(np.uint32)
    for name, (_, img) in runs.items():
        notes[name]["frame_bit_equal_to_single"] = bool(np.array_equal(img.cpu().numpy().view(np.uint32), want))
    for name, m in virt.items():
        st = [m.scene(r).lightmap_stats() for r in range(len(m.devices))]
        notes[name]["lightmap_stats_per_rank"] = st
        print(f"{name}: light samples / hits / deferred per rank: "
              + ", ".join(f"{s['samples']}/{s['hits']}/{s['deferred']}" for s in st))

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.reps

    ms = {name: [] for name in runs}
    names = list(runs)
    for r in range(a.rounds):  # every round starts one configuration further on: none keeps one place
        for name in names[r % len(names):] + names[:r % len(names)]:
            ms[name].append(wall(runs[name][0]))

    # the unpack of the 1-rank image alone, by device events
    g = torch.zeros((vrt.tiles_per_rank(film, 1) * 192,), device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    unpack = []
    for r in range(a.rounds + 1):
        e0.record(stream)
        for _ in range(a.reps):
            vrt.unpack_tiles_device(film, 1, g.data_ptr(), img_1.data_ptr(), sp)
        e1.record(stream)
        e1.synchronize()
        if r:
            unpack.append(e0.elapsed_time(e1) / a.reps)

    os.makedirs(a.out, exist_ok=True)
    lines = []
    for name in runs:
        lines.append({"config": name, **base, **notes[name], "frame_wall": summary(ms[name])})
    lines.append({"config": "unpack_1", **base, "what": "vrt_unpack_tiles_device of the 1-rank image, device events",
                  "kernel_events": summary(unpack)})
    ref = "single_parent" if a.parent else "single"
    d = np.array(ms["handle_1"]) - np.array(ms[ref])
    lines.append({"config": "handle_1_minus_" + ref, **base,
                  "what": "per round, the 1-rank handle's frame minus the single-scene frame of the same round",
                  "difference": summary(d.tolist()) if np.median(d) != 0 else {"ms_rounds": d.tolist()},
                  "reference_spread_ms": float(max(ms[ref]) - min(ms[ref])),
                  "unpack_ms_median": float(np.median(unpack))})
    with open(os.path.join(a.out, "multi_trace_bench.jsonl"), "w") as fh:
        for ln in lines:
            s = json.dumps(ln)
            print(s)
            fh.write(s + "\n")
    for m in handles:
        m.close()
    if a.parent:
        P.vrt_scene_destroy(ph)


if __name__ == "__main__":
    main()
