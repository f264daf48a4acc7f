#!/usr/bin/env python3
"""Timing of the light-probe gather (vrt_probe_gather_device) against the same
gather composed from the calls the library had before it: the probes' rays
prepared once on the device (outside the timed region),
vrt_trace_batch_device with parts.hits and parts.indirect, and the per-group
sum in torch (not bit-exact: only its time is used).

Workload: the bench's sponza-proxy with the light map of the driver's light
camera (VRT/main.cc:75-78), at each of --depths; probe sets (i) --probes
probes of radius 0.1 with origins uniform in the middle 80 % of the root box
and (ii) the reference driver's own 100 probes (VRT/main.cc:56-61).  Device
calls, HIP events on the stream after a warm-up, windows of >= --window
seconds, the two paths alternating inside every round.  The terms of the two
paths must be bit-identical at the timed sizes.

--parent LIB runs the composition through another libvrt.so (a build of the
parent commit) instead of the package's library.  --oracle-depth D also
times the CPU oracle's trace() over the 100 reference probes' rays at depth
D, as context.

usage: tools/probe_bench.py [--depths 6,8] [--probes 1024] [--rounds 5] [--out DIR]
"""
import argparse
import ctypes as C
import json
import math
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
f32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)


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


def bundle_rays(probes, points, res):
    """The gather's rays (n * 14 * npoints, 8) in float32, the operations of
    Ray{o, r_j + dirs_[i] * 2.6131f, r + res} (jql::dot's sum from zero)."""
    rd = points[None, :, :] + (vrt.PROBE_DIRS * f32(2.6131))[:, None, :]
    s = np.zeros(rd.shape[:2], np.float32)
    for k in range(3):
        s = s + rd[..., k] * rd[..., k]
    d = (rd / np.sqrt(s)[..., None]).astype(np.float32)
    n = len(probes)
    rays = np.zeros((n,) + d.shape[:2] + (8,), np.float32)
    rays[..., 0:3] = probes[:, None, None, :3]
    rays[..., 3:6] = d[None]
    rays[..., 6] = (probes[:, 3] + f32(res))[:, None, None]
    rays[..., 7] = FLT_MAX
    return rays.reshape(-1, 8)


def root_illum(tree, d):
    """root.compute_illum(d) (VRT/voxel_octree.h:72-82), the light colour the
    reference driver passes to gather_light (VRT/main.cc:105)."""
    key, _, ill = tree.lightmap_nodes()
    L = ill[0]  # the root: the smallest key
    dirs = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1)], np.float32)
    r = np.zeros(3, np.float32)
    for i in range(6):
        c = np.float32(0)
        for k in range(3):
            c = c + dirs[i, k] * d[k]
        r = r + L[i] * np.clip(c, f32(0), f32(1))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depths", default="6,8")
    ap.add_argument("--probes", type=int, default=1024)
    ap.add_argument("--radius", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--light-n", type=int, default=2048)
    ap.add_argument("--parent", default=None, help="a libvrt.so of the parent commit for the composed gather")
    ap.add_argument("--oracle-depth", type=int, default=0,
                    help="time the CPU oracle's trace() on the 100 reference probes' rays at this depth (0: not)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_gather"))
    a = ap.parse_args()

    L = vrt.lib()
    P = load(a.parent) if a.parent else L
    sd = vrt.SceneData.proxy(a.detail, 1)
    desc = sd.desc()
    lcam, lfilm = vrt.Camera(*LIGHT), vrt.Film(1, 1, a.light_n, a.light_n)
    points = vrt.probe_points()
    st = torch.cuda.current_stream().cuda_stream
    os.makedirs(a.out, exist_ok=True)
    results = {}
    for depth in [int(x) for x in a.depths.split(",")]:
        tree = vrt.VoxelOctree(sd, depth, device=0)
        tree.lightmap(lcam, lfilm)
        res = tree.min_voxel(depth)
        if P is L:
            ph = tree.h
        else:
            ph = C.c_void_p()
            ok(P, P.vrt_scene_create(C.byref(desc), depth, 0, C.byref(ph)), "vrt_scene_create (parent)")
            ok(P, P.vrt_lightmap_build(ph, C.byref(lcam.c), C.byref(lfilm.c), None), "vrt_lightmap_build (parent)")
        mn, mx = tree.root_box
        ctr, ext = (mn + mx) / 2, (mx - mn) / 2
        rng = np.random.default_rng(17)
        o = (ctr + rng.uniform(-0.8, 0.8, (a.probes, 3)) * ext).astype(f32)
        grid = np.concatenate([o, np.full((a.probes, 1), a.radius, f32)], axis=1)
        rp = vrt.probe_points(0xc01dbeefdeadbead, 100)  # VRT/main.cc:57-61
        ref100 = np.concatenate([rp + np.array((0.5, 0.4, 0.0), f32), np.full((100, 1), 0.1, f32)], axis=1).astype(f32)
        light = root_illum(tree, vrt.make_ray((0, 0, 0), (1, 10, 1))[3:6])  # VRT/main.cc:72,105
        lc = np.ascontiguousarray(light, f32)
        d_light = torch.from_numpy(lc).cuda()
        sets = {f"uniform{a.probes}": np.ascontiguousarray(grid), "reference100": np.ascontiguousarray(ref100)}
        out = {"min_voxel": res, "light_color": [float(x) for x in lc], "sets": {}}
        for sname, probes in sets.items():
            n = len(probes)
            nrays = n * 14 * 100
            d_probes = torch.from_numpy(probes).cuda()
            d_rays = torch.from_numpy(bundle_rays(probes, points, res)).cuda()
            d_sgs = torch.zeros((n, 14, 7), device="cuda")
            d_terms = torch.zeros((nrays, 3), device="cuda")
            d_rgb = torch.zeros((nrays, 3), device="cuda")
            d_hits = torch.zeros((nrays, 9), dtype=torch.int32, device="cuda")
            d_ind = torch.zeros((nrays, 3), device="cuda")
            parts = _ffi.TraceParts(d_hits.data_ptr(), d_ind.data_ptr(), None, None)
            comp = {}

            def new(terms=False):
                ok(L, L.vrt_probe_gather_device(tree.h, d_probes.data_ptr(), n, res, _ffi.ptr(lc, _ffi.f32p), None, 0,
                                                d_sgs.data_ptr(), d_terms.data_ptr() if terms else None, st),
                   "vrt_probe_gather_device")

            def composed():
                ok(P, P.vrt_trace_batch_device(ph, d_rays.data_ptr(), nrays, res, d_rgb.data_ptr(), C.byref(parts),
                                               st), "vrt_trace_batch_device")
                term = torch.where(d_hits[:, 0:1] != 0, d_ind, d_light)
                comp["terms"] = term
                comp["a"] = term.view(n, 14, 100, 3).sum(dim=2) / 100.0

            # the two paths compute the same terms at the timed size
            new(terms=True)
            composed()
            torch.cuda.synchronize()
            same = bool(torch.equal(comp["terms"].view(torch.int32), d_terms.view(torch.int32)))
            close = bool(torch.allclose(comp["a"], d_sgs[:, :, 0:3], rtol=1e-4, atol=1e-6, equal_nan=True))
            hit_share = float((d_hits[:, 0] != 0).float().mean())
            if not (same and close):
                raise SystemExit(f"depth {depth} {sname}: the composed gather and the new one differ "
                                 f"(terms identical {same}, amplitudes close {close})")

            def window(fn, reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / reps

            items = [("composed", composed), ("probe_gather", new)]
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
            out["sets"][sname] = {"probes": n, "rays": nrays, "hit_share": hit_share, "terms_identical": same,
                                  "calls_per_window": reps, "times": t,
                                  "composed_over_probe_gather": t["composed"]["ms_median"] / t["probe_gather"]["ms_median"],
                                  "mrays_per_s": nrays / t["probe_gather"]["ms_median"] / 1e3}
            if a.oracle_depth == depth and sname == "reference100":
                sys.path.insert(0, os.path.join(ROOT, "oracle"))
                import pyoracle as po
                osc = po.Scene(sd, depth)
                osc.lightmap(po.camera(*LIGHT), 1.0, 1.0, a.light_n, a.light_n, nthreads=16)
                rays = d_rays.cpu().numpy()
                t0 = time.perf_counter()
                osc.shade_trace(rays, res)
                out["sets"][sname]["cpu_oracle_trace_s"] = time.perf_counter() - t0
                osc.close()
        if P is not L:
            P.vrt_scene_destroy(ph)
        results[f"depth{depth}"] = out
        del tree
    doc = {"workload": {"detail": a.detail, "light_n": a.light_n, "radius": a.radius, "npoints": 100,
                        "rounds": a.rounds, "window_s": a.window, "device": torch.cuda.get_device_name(0),
                        "build_id": vrt.build_id(), "composition_library": a.parent or "package"},
           "results": results}
    with open(os.path.join(a.out, "probe_bench.json"), "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
