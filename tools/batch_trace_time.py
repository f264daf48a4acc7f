#!/usr/bin/env python3
"""Timing of the batched trace() (vrt_trace_batch_device) on the bench's trace
workload: depth 6, the proxy at bench detail, the light map `bench.py --mode
trace` builds.  Ray sets: (i) the 1024^2 main view's gen_rays4 rays in raster
order, (ii) the same rays permuted, (iii) a probe set (14 directions x 1,170
rays from one interior origin).  For (i) the frame call
(vrt_render_trace_device, same view, same light map) is timed in the same
run.  Device calls, HIP events after a warm-up, windows of >= --window
seconds, the items alternating inside every round.

Further libraries (`--variant build/ab/libvrt_X.so`, a `make variant` build of
another form of the cone kernel) are timed beside the package's library in
the same rounds, and every output of theirs (rgb, hits, the three parts) must
be byte-identical to the package library's.

usage: tools/batch_trace_time.py [--variant LIB ...] [--rounds 5] [--out FILE]
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


def ok(L, rc, where):
    if rc != 0:
        raise RuntimeError(f"{where}: {rc} {L.vrt_last_error().decode(errors='replace')}")


def view_rays(cam, film):
    """Every gen_rays4 ray of the film, index (py * nx + px) * 4 + s."""
    L = vrt.lib()
    out = np.zeros((film.ny * film.nx * 4, 8), np.float32)
    base = out.ctypes.data
    RP = C.POINTER(_ffi.Ray)
    for py in range(film.ny):
        for px in range(film.nx):
            L.vrt_gen_rays4(C.byref(cam.c), C.byref(film.c), px, py, C.cast(base + (py * film.nx + px) * 128, RP))
    return out


def probe_rays(mn, mx):
    rng = np.random.default_rng(11)
    o = ((mn + mx) / 2).astype(np.float32)
    o[1] = mn[1] + 0.4 * (mx[1] - mn[1])
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    dirs += [(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)]
    rays = []
    for d in dirs:
        dd = np.asarray(d, np.float64) / np.linalg.norm(d) + rng.normal(0, 0.35, (1170, 3))
        rays += [vrt.make_ray(o, x) for x in dd]
    return np.stack(rays)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", action="append", default=[], help="another libvrt.so build to time beside the package's")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--light-n", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_trace", "batch_trace.json"))
    a = ap.parse_args()

    paths = [vrt.LIB_PATH] + a.variant
    names = ["package"] + [os.path.basename(p) for p in a.variant]
    libs = [load(p) for p in paths]
    sd = vrt.SceneData.proxy(a.detail, 1)
    desc = sd.desc()
    film = vrt.Film(1.0, 1.0, a.size, a.size)
    cam, lcam, lfilm = vrt.Camera(*VIEW), vrt.Camera(*LIGHT), vrt.Film(1, 1, a.light_n, a.light_n)
    scenes = []
    for L in libs:
        h = C.c_void_p()
        ok(L, L.vrt_scene_create(C.byref(desc), a.depth, 0, C.byref(h)), "vrt_scene_create")
        ok(L, L.vrt_lightmap_build(h, C.byref(lcam.c), C.byref(lfilm.c), None), "vrt_lightmap_build")
        scenes.append(h)
    res = C.c_float()
    ok(libs[0], libs[0].vrt_scene_min_voxel(scenes[0], a.depth, C.byref(res)), "vrt_scene_min_voxel")
    res = res.value
    info = _ffi.SceneInfo()
    libs[0].vrt_scene_info(scenes[0], C.byref(info))
    mn, mx = np.array(info.root_min[:], np.float32), np.array(info.root_max[:], np.float32)

    raster = torch.from_numpy(view_rays(cam, film)).cuda()
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    sets = {"view_raster": raster, "view_permuted": raster[torch.randperm(len(raster), device="cuda", generator=g)],
            "probe": torch.from_numpy(probe_rays(mn, mx)).cuda()}
    nmax = len(raster)
    st = torch.cuda.current_stream().cuda_stream
    img = torch.zeros((a.size, a.size, 3), device="cuda")

    def outputs():
        return {"rgb": torch.zeros((nmax, 3), device="cuda"), "hits": torch.zeros((nmax, 9), dtype=torch.int32, device="cuda"),
                "indirect": torch.zeros((nmax, 3), device="cuda"), "direct": torch.zeros((nmax, 3), device="cuda"),
                "albedo": torch.zeros((nmax, 3), device="cuda")}

    def batch(k, rays, o, parts):
        pc = _ffi.TraceParts(o["hits"].data_ptr(), o["indirect"].data_ptr(), o["direct"].data_ptr(),
                             o["albedo"].data_ptr()) if parts else None
        ok(libs[k], libs[k].vrt_trace_batch_device(scenes[k], rays.data_ptr(), len(rays), res, o["rgb"].data_ptr(),
                                                   None if pc is None else C.byref(pc), st), "vrt_trace_batch_device")

    def frame():
        ok(libs[0], libs[0].vrt_render_trace_device(scenes[0], C.byref(cam.c), C.byref(film.c), res, 0, 1, 1,
                                                    img.data_ptr(), st), "vrt_render_trace_device")

    # output identity at the timed sizes (all parts), every library against the first
    o0, o1 = outputs(), outputs()
    identical = {}
    hit_share = {}
    for sname, rays in sets.items():
        batch(0, rays, o0, True)
        torch.cuda.synchronize()
        hit_share[sname] = float(o0["hits"][:len(rays), 0].float().mean())
        for k in range(1, len(libs)):
            for t in o1.values():
                t.zero_()
            batch(k, rays, o1, True)
            torch.cuda.synchronize()
            same = all(torch.equal(o0[key][:len(rays)].view(torch.int32), o1[key][:len(rays)].view(torch.int32))
                       for key in o0)
            identical[f"{names[k]}:{sname}"] = bool(same)
            if not same:
                raise SystemExit(f"{names[k]} differs from the package library on {sname}")
    del o1

    items = [(f"{names[k]}:{sname}", (lambda k=k, rays=rays: batch(k, rays, o0, False)))
             for sname, rays in sets.items() for k in range(len(libs))]
    items.append(("frame:view", frame))

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    reps = {}
    for name, fn in items:  # warm-up, and the calls a window needs
        window(fn, 2)
        reps[name] = max(3, math.ceil(a.window * 1000.0 / window(fn, 3)))
    ms = {name: [] for name, _ in items}
    for _ in range(a.rounds):
        for name, fn in items:
            ms[name].append(window(fn, reps[name]))

    def summary(v):
        med = float(np.median(v))
        return {"ms_median": med, "ms_rounds": [float(x) for x in v], "spread": float((max(v) - min(v)) / med)}

    out = {"workload": {"depth": a.depth, "detail": a.detail, "light_n": a.light_n, "size": a.size, "min_voxel": res,
                        "rays": {k: len(v) for k, v in sets.items()}, "hit_share": hit_share, "rounds": a.rounds,
                        "window_s": a.window, "calls_per_window": reps,
                        "device": torch.cuda.get_device_name(0), "build_id": vrt.build_id()},
           "times": {name: summary(v) for name, v in ms.items()},
           "outputs_identical": identical}
    f, b = out["times"]["frame:view"], out["times"]["package:view_raster"]
    out["view_raster_over_frame"] = b["ms_median"] / f["ms_median"]
    out["run_to_run_spread"] = max(f["spread"], b["spread"])
    for k in range(1, len(libs)):
        out[f"{names[k]}_over_package"] = {s: out["times"][f"{names[k]}:{s}"]["ms_median"] /
                                           out["times"][f"package:{s}"]["ms_median"] for s in sets}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    for L, h in zip(libs, scenes):
        L.vrt_scene_destroy(h)


if __name__ == "__main__":
    main()
