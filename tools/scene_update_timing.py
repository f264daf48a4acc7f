#!/usr/bin/env python3
"""Moving geometry: vrt_scene_update against destroy + create.

On the sponza-proxy (detail 1.0 by default) at depths 6, 8, 9 and 10, in one
process, alternating, best of three each:
  (a) destroy the scene, vrt_scene_create_ex(VRT_BUILD_DEVICE) on the moved
      positions -- what a caller had to do before vrt_scene_update;
  (b) vrt_scene_update from host arrays and vrt_scene_update_device from
      device arrays, on a second handle that lives through the whole run, to
      the positions (a) has just built from, with vrt_scene_update_stats'
      split.  That handle's first update, which allocates what later ones
      keep, is reported apart, and two more updates of each kind pass before
      the first one that counts.
The positions alternate between two rigid placements from round to round (the
moved one, the original, the moved one), and the updated handle always holds
the other placement, so every step rebuilds a different tree than the one it
starts from; "moved" is the best of the rounds on the moved placement for all
three, like against like.  One device build runs first at every depth and is
not counted (the first one in a process loads the code object).

  --lib PATH     load this libvrt.so instead of the package's (calls it lacks
                 are left out of the bindings)
  --create-only  (a) only: for a library from before the update call, to show
                 that the create path did not move
  --probes G     a probe scene: G x G x G light probes on a grid in the
                 triangles' box, moved with the placement, radius 0.1 x the
                 grid spacing.  (a) is vrt_scene_create_probes(VRT_BUILD_DEVICE |
                 VRT_BUILD_DEVICE_PROBES), (b) vrt_scene_update_probes[_device]
  --ranks N      the multi-device handle on N virtual ranks of device 0 (all
                 ranks share the one GPU: expect about N x a single update,
                 and nothing from the per-rank host threads).  (a) is
                 vrt_multi_destroy + vrt_scene_create_multi[_probes](VRT_BUILD_
                 DEVICE), (b) vrt_multi_update[_device] with vrt_multi_update_
                 stats' split, and one more update of each placement with
                 VRT_MULTI_UPDATE_VERIFY for the verify time
  --mask M       with or without --ranks: the handle on the real devices of
                 mask M (--ranks then must be left out)
Without --ranks / --mask the updated scene's vrt_scene_digest is timed too
(blocking call, best of five) and reported with the bytes it digests.
Prints and, with --out, writes one JSON document."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--depths", default="6,8,9,10")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lib")
    ap.add_argument("--create-only", action="store_true")
    ap.add_argument("--probes", type=int, default=0)
    ap.add_argument("--ranks", type=int, default=0)
    ap.add_argument("--mask", type=lambda x: int(x, 0), default=0)
    ap.add_argument("--out")
    a = ap.parse_args()
    multi = bool(a.ranks or a.mask)
    if a.ranks and a.mask:
        ap.error("--ranks (virtual ranks on device 0) and --mask (real devices) exclude each other")

    import torch  # first: one HIP runtime per process
    from voxelraytrace20190722_amd import _ffi
    if a.lib:
        import ctypes
        _ffi.LIB_PATH = os.path.abspath(a.lib)
        older = ctypes.CDLL(_ffi.LIB_PATH)  # an older library lacks the newer symbols
        for name in [n for n in _ffi.SIGNATURES if not hasattr(older, n)]:
            del _ffi.SIGNATURES[name]
    import voxelraytrace20190722_amd as vrt

    sd = vrt.SceneData.proxy(a.detail, 1)
    p3 = sd.pos.reshape(-1, 3)
    c, s = np.float32(np.cos(0.3)), np.float32(np.sin(0.3))
    R = np.array(((c, 0, s), (0, 1, 0), (-s, 0, c)), np.float32)
    places = [sd.pos,
              np.ascontiguousarray((p3 @ R.T + np.array((0.5, 0.25, -0.5), np.float32)).astype(np.float32)
                                   .reshape(-1, 9))]
    scenes = [vrt.SceneData(p, sd.nrm, sd.uv, sd.mat, sd.mat_tex, sd.mat_kd, sd.tex_dims, sd.tex_off, sd.tex_data)
              for p in places]
    d_places = [torch.from_numpy(p).cuda() for p in places]
    probes = d_probes = None
    if a.probes:
        g = a.probes
        mn, mx = p3.min(axis=0), p3.max(axis=0)
        cell = (mx - mn) / np.float32(g)
        ijk = np.stack(np.meshgrid(*[np.arange(g)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
        o = (mn + (ijk + np.float32(0.5)) * cell).astype(np.float32)
        r = np.full((len(o), 1), np.float32(0.1) * cell.min(), np.float32)
        probes = [np.ascontiguousarray(np.concatenate([o, r], axis=1)),
                  np.ascontiguousarray(np.concatenate(
                      [(o @ R.T + np.array((0.5, 0.25, -0.5), np.float32)).astype(np.float32), r], axis=1))]
        d_probes = [torch.from_numpy(p).cuda() for p in probes]
    torch.cuda.synchronize()
    doc = {"scene": "sponza-proxy", "detail": a.detail, "triangles": int(sd.ntri), "reps": a.reps,
           "probes": 0 if probes is None else int(len(probes[0])),
           "library": vrt.build_id(), "device": torch.cuda.get_device_name(0), "depths": {}}
    if multi:
        doc["ranks"] = a.ranks if a.ranks else bin(a.mask).count("1")
        doc["virtual_ranks"] = bool(a.ranks)

    def make(k, depth):
        if multi:
            return vrt.MultiOctree(scenes[k], depth, device_mask=a.mask or 1, build_on_device=True,
                                   virtual_ranks=a.ranks or None, probes=None if probes is None else probes[k])
        return vrt.VoxelOctree(scenes[k], depth, build_on_device=True, probes=None if probes is None else probes[k])

    def timed_update(live, kind, k, verify=False):
        t0 = time.perf_counter()
        if multi:
            if kind == "host":
                live.update(places[k], None, None if probes is None else probes[k], verify=verify)
            else:
                live.update_device(d_places[k].data_ptr(), None, None if probes is None else d_probes[k].data_ptr(),
                                   verify=verify)
        elif probes is not None:
            if kind == "host":
                live.update_probes(places[k], None, probes[k])
            else:
                live.update_probes_device(d_places[k].data_ptr(), None, d_probes[k].data_ptr())
        elif kind == "host":
            live.update(places[k])
        else:
            live.update_device(d_places[k].data_ptr())
        return dict(live.update_stats(), wall=(time.perf_counter() - t0) * 1e3, placement=k)

    def pinfo(t):
        return (t.scene(0) if multi else t).probe_info()

    for depth in [int(x) for x in a.depths.split(",")]:
        tree = make(0, depth)  # warm-up, not counted
        create, upd, upd_dev = [], [], []
        live = first = None
        if not a.create_only:
            # the handle that is updated lives through the depth's whole run.
            # Its first update allocates the build's scratch and the host
            # mirrors' second halves and is reported apart; one update of each
            # kind after it is not counted, the rest are the steady state.
            live = make(0, depth)
            first = timed_update(live, "host", 1)
            timed_update(live, "device", 0)
            timed_update(live, "host", 1)
            timed_update(live, "device", 0)
        k = 0
        for _ in range(a.reps):
            k ^= 1  # this round's positions: 1, 0, 1, ... for (a) and (b) alike
            t0 = time.perf_counter()
            tree.close()
            tree = make(k, depth)
            create.append({"total": (time.perf_counter() - t0) * 1e3, "build_ms": tree.info.build_ms,
                           "upload_ms": tree.info.upload_ms, "gpu": tree.info.build_device_ms, "placement": k})
            if a.create_only:
                continue
            # live holds the other placement: each update rebuilds the tree
            # (a) has just built, from a different one; between the two it is
            # moved back, not counted
            upd.append(timed_update(live, "host", k))
            timed_update(live, "host", k ^ 1)
            upd_dev.append(timed_update(live, "device", k))
            assert int(live.info.nodes) == int(tree.info.nodes) and int(live.info.tri_refs) == int(tree.info.tri_refs)
            assert pinfo(live) == pinfo(tree)
        row = {"nodes": int(tree.info.nodes), "tri_refs": int(tree.info.tri_refs),
               "probe_leaves": int(pinfo(tree)[1]), "probe_refs": int(pinfo(tree)[2]),
               "create": min(create, key=lambda r: r["total"])}
        if not a.create_only:
            row["update_first"] = first
            row["update"] = min(upd, key=lambda r: r["wall"])
            row["update_device"] = min(upd_dev, key=lambda r: r["wall"])
            # like against like: the best of the rounds on the moved positions
            row["moved"] = {"create": min(r["total"] for r in create if r["placement"] == 1),
                            "update": min(r["wall"] for r in upd if r["placement"] == 1),
                            "update_device": min(r["wall"] for r in upd_dev if r["placement"] == 1)}
            if multi:
                # the replica check: one more update of each kind with the flag
                row["verify"] = {"update": timed_update(live, "host", 1, verify=True),
                                 "update_device": timed_update(live, "device", 0, verify=True)}
                row["update_scratch_bytes"] = int(live.scene(0).update_scratch())
            elif "vrt_scene_digest" not in _ffi.SIGNATURES:  # an older library
                row["update_scratch_bytes"] = int(live.update_scratch())
            else:
                walls = []
                for _ in range(5):
                    t0 = time.perf_counter()
                    live.digest()
                    walls.append((time.perf_counter() - t0) * 1e3)
                nb = sum(int(live.device_array(kk).size) for kk in range(5 if probes is None else 8))
                row["digest"] = {"wall_ms": min(walls), "bytes": nb + int(live.info.nodes) * 36}
                row["update_scratch_bytes"] = int(live.update_scratch())
            row["device_bytes"] = int(live.info.device_bytes)
            row["rounds"] = {"create": create, "update": upd, "update_device": upd_dev}
            live.close()
        doc["depths"][str(depth)] = row
        tree.close()
        print(f"depth {depth}: " + json.dumps(row), flush=True)
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
