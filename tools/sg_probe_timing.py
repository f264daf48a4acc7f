#!/usr/bin/env python3
"""The SG algebra and the probes' irradiance on the device against what a
caller compares them with.

On the committed scene_proxy.npz at depth 8 with 100 light probes of radius
0.1 (centres from reference_gi_cases.scene_probes) and seeded stored SGs, at
--n elements (default 2^20), in one process, after a warm-up, the median of
--reps repetitions (default 5), HIP events around each call on one stream:
  inner      vrt_sg_inner_prod_device over n random SG pairs
  irradiance vrt_probe_irradiance_device at n points drawn uniformly in the
             root box, random unit normals, the cosine lobe
  cones      vrt_cone_trace_batch_device at the same points and normals (the
             cost "light from the probes" is compared with; needs a light map)
and, with a host clock, the host calls on the same inputs:
  inner_host       vrt_sg_inner_prod
  irradiance_host  vrt_probe_irradiance (up to 16 threads)
The device results are compared with the host calls' in bits (NaN matching
NaN) before anything is timed.  Prints and, with --out, writes one JSON
document."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: one HIP runtime per process)

import voxelraytrace20190722_amd as vrt  # noqa: E402
import reference_gi_cases as rc  # noqa: E402

F = np.float32


def same(a, b):
    return bool(np.all((np.isnan(a) & np.isnan(b)) | (a.view(np.uint32) == b.view(np.uint32))))


def device_ms(call, st, reps, warmup=2):
    for _ in range(warmup):
        call()
    st.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        call()
        e1.record(st)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def host_ms(call, reps):
    call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def summary(ms, n):
    med = statistics.median(ms)
    return {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "ns_per_element": med * 1e6 / n,
            "all_ms": [round(v, 4) for v in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--probes", type=int, default=100)
    ap.add_argument("--radius", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    n = args.n
    z = np.load(os.path.join(rc.GOLDEN, "scene_proxy.npz"), allow_pickle=False)
    sd = rc.scene_from(z)
    v = np.asarray(sd.pos, F).reshape(-1, 3)
    probes = rc.scene_probes(v.min(axis=0), v.max(axis=0), n=args.probes)
    probes[:, 3] = args.radius
    tree = vrt.VoxelOctree(sd, args.depth, probes=probes)
    rng = np.random.default_rng(7)
    d = vrt.PROBE_DIRS / np.linalg.norm(vrt.PROBE_DIRS, axis=1, keepdims=True)
    tree.probe_sgs = {"a": rng.uniform(0, 2, (args.probes, 14, 3)).astype(F),
                      "d": np.tile(d.astype(F), (args.probes, 1, 1)), "s": np.full((args.probes, 14), 10, F)}
    assert tree.lightmap(vrt.Camera(*rc.LIGHT), vrt.Film(1, 1, 256, 256)) > 0
    mn, mx = tree.root_box
    p = (mn + rng.uniform(0, 1, (n, 3)) * (mx - mn)).astype(F)
    p = np.minimum(np.maximum(p, mn), mx)
    isects = np.ascontiguousarray(np.concatenate([p, rc.unit_dirs(8, n)], axis=1))
    reps = -(-n // 512)
    lhs, rhs, _ = rc.sg_pairs(12, 512)
    lhs, rhs = np.tile(lhs, (reps, 1))[:n], np.tile(rhs, (reps, 1))[:n]
    lhs[:, 0:3] = rng.uniform(0, 2, (n, 3)).astype(F)  # not 2,048 copies of one batch's amplitudes
    lhs, rhs = np.ascontiguousarray(lhs), np.ascontiguousarray(rhs)

    dev = lambda a: torch.from_numpy(a).cuda()
    d_lhs, d_rhs, d_is = dev(lhs), dev(rhs), dev(isects)
    d_inner, d_irr, d_cone = (torch.zeros((n, 3), device="cuda") for _ in range(3))
    d_cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    res = tree.min_voxel()
    calls = {
        "inner": lambda: vrt.sg_inner_prod_device(d_lhs.data_ptr(), d_rhs.data_ptr(), n, d_inner.data_ptr(), 0,
                                                  st.cuda_stream),
        "irradiance": lambda: tree.probe_irradiance_device(d_is.data_ptr(), n, d_irr.data_ptr(), d_cnt.data_ptr(),
                                                           stream_ptr=st.cuda_stream),
        "cones": lambda: tree.cone_trace_device(d_is.data_ptr(), n, d_cone.data_ptr(), res, st.cuda_stream),
    }
    torch.cuda.synchronize()
    for c in calls.values():
        c()
    st.synchronize()
    want_inner = vrt.sg_inner_prod(lhs, rhs)
    want_irr, want_cnt = tree.probe_irradiance(isects[:, 0:3], isects[:, 3:6], counts=True)
    assert same(d_inner.cpu().numpy(), want_inner), "inner_prod: device != host"
    assert same(d_irr.cpu().numpy(), want_irr) and np.array_equal(d_cnt.cpu().numpy(), want_cnt), \
        "irradiance: device != host"
    out = {"scene": "scene_proxy.npz", "depth": args.depth, "probes": args.probes, "radius": args.radius, "n": n,
           "reps": args.reps, "nodes": int(tree.info.nodes), "probe_info": list(tree.probe_info()),
           "count_histogram": np.bincount(want_cnt).tolist(), "expf_flavour": vrt.expf_flavour(),
           "build": vrt.build_id()}
    for k, c in calls.items():
        out[k] = summary(device_ms(c, st, args.reps), n)
    out["inner_host"] = summary(host_ms(lambda: vrt.sg_inner_prod(lhs, rhs), min(args.reps, 3)), n)
    out["irradiance_host"] = summary(host_ms(lambda: tree.probe_irradiance(isects[:, 0:3], isects[:, 3:6]),
                                             min(args.reps, 3)), n)
    out["irradiance_over_cones"] = out["irradiance"]["median_ms"] / out["cones"]["median_ms"]
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
