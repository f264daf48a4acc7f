"""The allocations a scene keeps between calls, through every path that grows
one: each call runs at a small size, at a larger one (the kept allocation is
released and made anew) and at the small size again (the larger one is
reused), and every result must equal, bit for bit, the same call on a fresh
scene that never grew.  After the sequence vrt_scene_scratch_bytes reports what
it reported when the numbers below were recorded; then the scenes are
destroyed and a new one is made and used in the same process.

One triangle scene and one probe scene (scene_proxy.npz at depth 3):
  vrt_render to a host image (the device image and its pinned copy),
  vrt_ray_march_batch (the ray / hit staging),
  vrt_trace_batch with parts and vrt_probe_gather with terms under the small
  chunk flags (the batched staging; three chunks and more, a ragged last one),
  vrt_render_trace[_probes] (a trace set's records, the step table after them),
  vrt_render_secondary (a compaction set),
  vrt_render_tiles_device as ranks 0 and 1 of 2 on one GPU (the deal maps).
A failed launch followed by a good one is test_gpu_frames.py::
test_failed_launch_leaves_work_queue_usable."""
import numpy as np
import pytest
import torch

import voxelraytrace20190722_amd as vrt

import probe_cases as pc
from test_frame_args_gpu import DEPTH, N, Scenes, film

pytestmark = pytest.mark.gpu

SMALL, LARGE = 5, 401  # batch elements: one chunk; 200 + 200 + 1 rays, 201 chunks of probes
NPTS = 4
# vrt_scene_scratch_bytes (total, compaction) after the sequence, recorded on an MI355X before the scene's device
# resources got their owners
SCRATCH = {"tri": (101390320, 100979712), "probe": (101390320, 100979712)}


@pytest.fixture(scope="module")
def sc():
    s = Scenes()
    f = film(32, 32)
    rays = np.concatenate([s.cam.gen_rays4(f, px, py) for py in range(0, 32, 3) for px in range(0, 32, 3)])
    s.rays = np.ascontiguousarray(np.resize(rays, (LARGE, 8)), np.float32)
    ctr, r = s.probes[0, :3], s.probes[0, 3]
    k = np.arange(LARGE, dtype=np.float32)[:, None]
    s.gprobes = np.concatenate([ctr + 0.001 * r * k * np.array((1, -1, 0.5), np.float32), np.full((LARGE, 1), r)],
                               axis=1).astype(np.float32)
    s.points = vrt.probe_points(7, NPTS)
    return s


def fresh(sc, kind):
    t = vrt.VoxelOctree(sc.sd, DEPTH, probes=sc.probes if kind == "probe" else None)
    assert t.lightmap(sc.light, film()) > 0
    if kind == "probe":
        t.gather_probes(0.0, (1.0, 0.9, 0.8))
    return t


def flat(x):
    """A call's result as a list of uint32 arrays."""
    if isinstance(x, dict):
        return [a for k in sorted(x) for a in flat(x[k])]
    if isinstance(x, (tuple, list)):
        return [a for v in x for a in flat(v)]
    if isinstance(x, np.ndarray):
        return [pc.bits(x.astype(np.float32) if x.dtype == np.float64 else x) if x.dtype.itemsize == 4 else x]
    return [np.asarray(x)]


def tiles_2ranks(tree, sc, n):
    f = film(n, n)
    out = []
    for rank in (0, 1):
        d = torch.zeros(vrt.tiles_per_rank(f, 2) * 64 * 3, device="cuda")
        torch.cuda.synchronize()
        tree.render_tiles_device(sc.cam, f, rank, 2, 0, d.data_ptr(), None)
        torch.cuda.synchronize()
        out.append(d.cpu().numpy())
    return out


def chunked(flag, call):
    try:
        vrt.set_test_flags(flag)
        return call()
    finally:
        vrt.set_test_flags(0)


def paths(sc, kind):
    """name -> (call(tree, size), sizes small / large)"""
    trace = "render_trace_probes" if kind == "probe" else "render_trace"
    return {
        "render": (lambda t, n: t.render(sc.cam, film(n, n)), (N, 24)),
        "ray_march": (lambda t, n: t.ray_march(sc.rays[:n], even_invisible=kind == "probe"), (8, 200)),
        "trace": (lambda t, n: chunked(vrt.TEST_SMALL_BATCH_CHUNK, lambda: t.trace(sc.rays[:n], parts=True)),
                  (SMALL, LARGE)),
        "gather": (lambda t, n: chunked(vrt.TEST_SMALL_PROBE_CHUNK,
                                        lambda: t.probe_gather(sc.gprobes[:n], 0.0, (1.0, 0.9, 0.8), sc.points,
                                                               terms=True)), (SMALL, LARGE)),
        trace: (lambda t, n: getattr(t, trace)(sc.cam, film(n, n), samples=True), (N, 32)),
        "secondary": (lambda t, n: t.render_secondary(sc.cam, film(n, n), 64, ids="hit"), (N, 32)),
        "tiles": (lambda t, n: tiles_2ranks(t, sc, n), (32, 48)),
    }


@pytest.mark.parametrize("kind", ["tri", "probe"])
def test_grown_scene_equals_fresh_scenes(sc, kind):
    P = paths(sc, kind)
    # every call on a scene of its own, which never grew
    want = {(name, n): flat(call(fresh(sc, kind), n)) for name, (call, sizes) in P.items() for n in sizes}
    tree = fresh(sc, kind)
    for rnd in range(2):  # the second round finds every allocation at its largest
        for name, (call, (small, large)) in P.items():
            for n in (small, large, small):
                got = flat(call(tree, n))
                assert len(got) == len(want[name, n])
                for a, b in zip(got, want[name, n]):
                    assert np.array_equal(a, b), (kind, rnd, name, n)
    assert any(a.any() for a in want["render", N]) and any(a.any() for a in want["trace", LARGE])
    got = tree.scratch_bytes()
    print(f"scratch_bytes[{kind}] = {got}")
    assert got == SCRATCH[kind], (kind, got)
    # destroy, then a new scene in the same process
    tree.close()
    t2 = fresh(sc, kind)
    for name in ("render", "trace"):
        call, (small, _) = P[name]
        for a, b in zip(flat(call(t2, small)), want[name, small]):
            assert np.array_equal(a, b), (kind, "after destroy", name)
    t2.close()
