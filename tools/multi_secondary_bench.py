#!/usr/bin/env python3
"""Timing of one rank's config-5 share with the share-sized primary pass
(vrt_render_secondary_tiles_device) against the share step it replaces
(vrt_render_secondary_device, whose primary pass covers the whole film, +
vrt_pack_tiles_c_device), for every rank of --ranks on ONE GPU.  Scene and view
are bench.py --mode secondary's: the sponza-proxy at --depth, --width x
--height, --spp rays per hit pixel, the sweep poses in turn.

What is timed, in windows of --reps frames (pose k % poses for frame k) that
alternate inside every round, each round starting one configuration further on
(median and [min, max] of the rounds; a device synchronise closes every window;
every configuration is warmed up and its output compared bit for bit first):

  share_tiles r    this tree's vrt_render_secondary_tiles_device, rank r.
  share_whole r    this tree's vrt_render_secondary_device + vrt_pack_tiles_c_device:
                   the same kernels as the parent's, a control for the library load.
  share_parent r   with --parent LIB (a libvrt.so built from the parent commit,
                   loaded beside this tree's): the parent's share step.
  one_rank         vrt_render_secondary_device, rank 0 of 1: the whole frame.
  handle_n         vrt_render_secondary_multi_device on n virtual ranks: n
                   replicas on ONE GPU, the gather done by device copies.  A
                   rehearsal of the code path, not a scaling result; no transfer
                   between devices is measured by this tool.

One JSON line per configuration and a summary line, printed and written to
--out/multi_secondary_bench.jsonl.

usage: tools/multi_secondary_bench.py [--depth 8] [--width 1920] [--height 1080] [--spp 64] [--ranks 8]
                                      [--rounds 7] [--reps 16] [--parent LIB] [--out DIR]
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
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--poses", type=int, default=16)
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=16, help="frames per timed window")
    ap.add_argument("--parent", default=None, help="a libvrt.so of the parent commit: its share step too")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_secondary"))
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds: the median of at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool only measures on one")

    n = a.ranks
    sd = vrt.SceneData.proxy(a.detail, 1)
    tree = vrt.VoxelOctree(sd, a.depth, device=0)
    mn, mx = tree.root_box
    cams = [vrt.Camera(*vrt.sweep_pose(mn, mx, i, a.poses)) for i in range(a.poses)]
    film = vrt.Film(1, 1, a.width, a.height)
    nx, ny = a.width, a.height
    w8, h8 = nx // 8 * 8, ny // 8 * 8
    tpr = vrt.tiles_per_rank(film, n)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    base = {"device": torch.cuda.get_device_name(0), "build_id": vrt.build_id(), "depth": a.depth, "width": nx,
            "height": ny, "spp": a.spp, "detail": a.detail, "ranks": n, "rounds": a.rounds,
            "frames_per_window": a.reps, "poses": a.poses}

    def f32(*shape):
        return torch.zeros(shape, dtype=torch.float32, device="cuda")

    runs, notes = {}, {}

    def add(name, fn, **extra):
        runs[name] = fn
        notes[name] = extra

    P = ph = None
    if a.parent:
        P = load(a.parent)
        ph, desc = C.c_void_p(), sd.desc()
        rc = P.vrt_scene_create_ex(C.byref(desc), a.depth, 0, 0, C.byref(ph))
        if rc != 0:
            raise RuntimeError(f"parent vrt_scene_create_ex: {rc} {P.vrt_last_error().decode(errors='replace')}")
        base["parent_build_id"] = P.vrt_build_id().decode()

    packed = {}
    for r in range(n):
        prim_t, vis_t, pk_t = f32(w8 * h8 * 8), f32(ny, nx), f32(tpr * 64)
        hits = torch.zeros(1, dtype=torch.int64, device="cuda")
        packed[("tiles", r)] = pk_t
        add(f"share_tiles_{r}", (lambda k, r=r, p=prim_t, v=vis_t, q=pk_t, h=hits: tree.render_secondary_tiles_device(
            cams[k % a.poses], film, a.spp, r, n, p.data_ptr(), v.data_ptr(), q.data_ptr(), h.data_ptr(), sp)),
            what="vrt_render_secondary_tiles_device: share-sized primary pass + walk + pack", rank=r)
        prim_w, vis_w, pk_w = f32(w8 * h8 * 8), f32(ny, nx), f32(tpr * 64)
        packed[("whole", r)] = pk_w

        def whole(k, r=r, p=prim_w, v=vis_w, q=pk_w):
            tree.render_secondary_device(cams[k % a.poses], film, a.spp, r, n, p.data_ptr(), v.data_ptr(), sp)
            vrt.pack_tiles_c_device(film, r, n, 1, v.data_ptr(), q.data_ptr(), sp)
        add(f"share_whole_{r}", whole, rank=r,
            what="this tree's vrt_render_secondary_device (whole-film primary pass) + vrt_pack_tiles_c_device")
        if P:
            prim_p, vis_p, pk_p = f32(w8 * h8 * 8), f32(ny, nx), f32(tpr * 64)
            packed[("parent", r)] = pk_p

            def parent(k, r=r, p=prim_p, v=vis_p, q=pk_p):
                cam = cams[k % a.poses]
                rc = P.vrt_render_secondary_device(ph, C.byref(cam.c), C.byref(film.c), a.spp, r, n,
                                                   C.c_void_p(p.data_ptr()), C.c_void_p(v.data_ptr()), C.c_void_p(sp))
                rc = rc or P.vrt_pack_tiles_c_device(C.byref(film.c), r, n, 1, C.c_void_p(v.data_ptr()),
                                                     C.c_void_p(q.data_ptr()), C.c_void_p(sp))
                if rc != 0:
                    raise RuntimeError(f"parent share step: {rc}")
            add(f"share_parent_{r}", parent, rank=r,
                what="the parent commit's library: vrt_render_secondary_device + vrt_pack_tiles_c_device")
    prim_1, img_1 = f32(w8 * h8 * 8), f32(ny, nx)
    add("one_rank", lambda k: tree.render_secondary_device(cams[k % a.poses], film, a.spp, 0, 1, prim_1.data_ptr(),
                                                           img_1.data_ptr(), sp),
        what="vrt_render_secondary_device, rank 0 of 1: the frame of bench.py --mode secondary")
    m = vrt.MultiOctree(sd, a.depth, device_mask=1, virtual_ranks=n)
    img_m = f32(ny, nx)
    add(f"handle_{n}", lambda k: m.render_secondary_device(cams[k % a.poses], film, a.spp, img_m.data_ptr(), sp),
        what="vrt_render_secondary_multi_device on virtual ranks: n replicas on ONE GPU, a rehearsal of the code "
             "path, not a scaling result; no transfer between devices is measured", virtual_ranks=n)

    # warm-up, then every configuration's output for pose 0 against the one-rank image's tiles
    for fn in runs.values():
        for k in (1, 2, 0):
            fn(k)
    torch.cuda.synchronize()
    one = img_1.cpu().numpy()
    rank_of, slot_of = vrt.tile_deal_map(film, n)
    tiles = one[:h8, :w8].reshape(h8 // 8, 8, w8 // 8, 8).transpose(0, 2, 1, 3)
    for (kind, r), buf in packed.items():
        cnt = int((rank_of == r).sum())
        want = np.zeros((cnt, 64), np.float32)
        want[slot_of[rank_of == r]] = tiles[rank_of == r].reshape(cnt, 64)
        same = bool(np.array_equal(buf.cpu().numpy()[:cnt * 64].view(np.uint32), want.ravel().view(np.uint32)))
        notes[f"share_{kind}_{r}"].update(tiles=cnt, packed_bit_equal_to_one_rank_image=same)
    notes[f"handle_{n}"]["frame_bit_equal_to_one_rank"] = bool(
        np.array_equal(img_m.cpu().numpy().view(np.uint32), one.view(np.uint32)))

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(a.reps):
            fn(k)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.reps

    ms = {name: [] for name in runs}
    names = list(runs)
    for r in range(a.rounds):  # every round starts one configuration further on: none keeps one place
        for name in names[r % len(names):] + names[:r % len(names)]:
            ms[name].append(wall(runs[name]))

    lines = [{"config": name, **base, **notes[name], "frame_wall": summary(ms[name])} for name in runs]
    med = {name: float(np.median(v)) for name, v in ms.items()}
    ref = "parent" if P else "whole"
    slow_new = max(range(n), key=lambda r: med[f"share_tiles_{r}"])
    slow_ref = max(range(n), key=lambda r: med[f"share_{ref}_{r}"])
    lines.append({
        "config": "summary", **base, "reference": f"share_{ref}",
        "per_rank_ms": [{"rank": r, "tiles_ms": med[f"share_tiles_{r}"], "reference_ms": med[f"share_{ref}_{r}"],
                         "saved_ms": med[f"share_{ref}_{r}"] - med[f"share_tiles_{r}"],
                         "reference_min_max": [float(min(ms[f"share_{ref}_{r}"])), float(max(ms[f"share_{ref}_{r}"]))],
                         "tiles_min_max": [float(min(ms[f"share_tiles_{r}"])), float(max(ms[f"share_tiles_{r}"]))]}
                        for r in range(n)],
        "slowest_share_tiles": {"rank": slow_new, "ms": med[f"share_tiles_{slow_new}"]},
        "slowest_share_reference": {"rank": slow_ref, "ms": med[f"share_{ref}_{slow_ref}"]},
        "one_rank_ms": med["one_rank"],
        "one_rank_over_slowest_share_tiles": med["one_rank"] / med[f"share_tiles_{slow_new}"],
        "one_rank_over_slowest_share_reference": med["one_rank"] / med[f"share_{ref}_{slow_ref}"],
        f"handle_{n}_ms": med[f"handle_{n}"],
    })
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "multi_secondary_bench.jsonl"), "w") as fh:
        for ln in lines:
            s = json.dumps(ln)
            print(s)
            fh.write(s + "\n")
    m.close()
    if P:
        P.vrt_scene_destroy(ph)


if __name__ == "__main__":
    main()
