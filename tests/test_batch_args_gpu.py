"""What the batched calls refuse, and with what: the status and a piece of
vrt_last_error() for every rejected call of vrt_trace_batch,
vrt_cone_trace_batch, vrt_probe_gather and their _device forms, on a triangle
scene, a probe scene and a host-only scene; and which refusal answers where two
apply at once.  The sibling of test_frame_args_gpu.py, on the same scenes.
Every call here is refused on the host before anything is launched, or is a
valid call over 8 elements.

A NaN min_voxel is no refusal: like every min_voxel that is not > 0 it stands
for the scene's own, so the call is the valid call; an infinite one is the
degenerate cone step."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import voxelraytrace20190722_amd as vrt
from voxelraytrace20190722_amd import _ffi

import probe_cases as pc
from test_frame_args_gpu import DEPTH, N, Scenes, film

pytestmark = pytest.mark.gpu

OK, INVALID, NODEVICE = _ffi.VRT_OK, _ffi.VRT_E_INVALID, _ffi.VRT_E_NODEVICE
TRACE = ("vrt_trace_batch", "vrt_trace_batch_device")
CONE = ("vrt_cone_trace_batch", "vrt_cone_trace_batch_device")
GATHER = ("vrt_probe_gather", "vrt_probe_gather_device")
BATCH = TRACE + CONE + GATHER
NEL = 8  # elements of a valid call
NPTS = 4  # sample points of a gather that brings its own


@pytest.fixture(scope="module")
def sc():
    s = Scenes()
    # 8 rays into the scene, the hit points and normals of those that hit (else a point of the box), 8 probes
    s.rays = np.concatenate([s.cam.gen_rays4(film(), px, py) for py in (3, 9) for px in (2, 12)])[:NEL]
    s.rays = np.ascontiguousarray(s.rays, np.float32)
    h = s.tri.ray_march(s.rays)
    s.isects = np.ascontiguousarray(np.concatenate([h["hit_p"], h["normal"]], axis=1), np.float32)
    s.gprobes = np.ascontiguousarray(np.repeat(s.probes, NEL // len(s.probes), axis=0), np.float32)
    s.points = vrt.probe_points(7, NPTS)
    return s


class Call:
    """One call of a batched entry point: the valid arguments over NEL
    elements, changed by keyword.  inp / rgb / sgs / light / parts: False
    passes a null pointer; points: True passes NPTS sample points with
    `npoints` as their count."""

    def __init__(self, sc, tree, name, **kw):
        a = dict(scene=True, n=NEL, inp=True, rgb=True, sgs=True, light=True, parts=False, points=False, npoints=NPTS,
                 terms=False, min_voxel=0.0)
        a.update(kw)
        L = _ffi.lib()
        dev = name.endswith("_device")
        h = tree.h if a["scene"] and tree is not None else None
        src = sc.rays if name in TRACE else sc.isects if name in CONE else sc.gprobes
        outs = {"rgb": np.zeros((NEL, 3), np.float32), "sgs": np.zeros((NEL, 14, 7), np.float32),
                "terms": np.zeros((NEL, 14, NPTS, 3), np.float32), "hits": np.zeros((NEL, 9), np.float32),
                "indirect": np.zeros((NEL, 3), np.float32), "direct": np.zeros((NEL, 3), np.float32),
                "albedo": np.zeros((NEL, 3), np.float32)}
        if dev:
            d_src = torch.from_numpy(src).cuda()
            d_out = {k: torch.from_numpy(v).cuda() for k, v in outs.items()}
            torch.cuda.synchronize()
            p_in = C.c_void_p(d_src.data_ptr())
            vp = lambda k: C.c_void_p(d_out[k].data_ptr())
            addr = lambda k: d_out[k].data_ptr()
        else:
            vp = lambda k: outs[k].ctypes.data_as(_ffi.f32p)
            addr = lambda k: outs[k].ctypes.data
        mv = C.c_float(a["min_voxel"])
        n = a["n"]
        if name in TRACE:
            parts = _ffi.TraceParts(addr("hits"), addr("indirect"), addr("direct"), addr("albedo")) if a["parts"] else None
            pp = None if parts is None else C.byref(parts)
            if dev:
                self.status = L.vrt_trace_batch_device(h, p_in if a["inp"] else None, n, mv, vp("rgb") if a["rgb"] else None,
                                                       pp, None)
            else:
                self.status = L.vrt_trace_batch(h, src.ctypes.data_as(C.POINTER(_ffi.Ray)) if a["inp"] else None, n, mv,
                                                vp("rgb") if a["rgb"] else None, pp)
        elif name in CONE:
            if dev:
                self.status = L.vrt_cone_trace_batch_device(h, p_in if a["inp"] else None, n, mv,
                                                            vp("rgb") if a["rgb"] else None, None)
            else:
                self.status = L.vrt_cone_trace_batch(h, src.ctypes.data_as(C.POINTER(_ffi.ISect)) if a["inp"] else None, n,
                                                     mv, vp("rgb") if a["rgb"] else None)
        else:
            lc = _ffi.ptr(np.array((1.0, 0.9, 0.8), np.float32), _ffi.f32p) if a["light"] else None
            pts = _ffi.ptr(sc.points, _ffi.f32p) if a["points"] else None
            if dev:
                self.status = L.vrt_probe_gather_device(h, p_in if a["inp"] else None, n, mv, lc, pts, a["npoints"],
                                                        vp("sgs") if a["sgs"] else None,
                                                        vp("terms") if a["terms"] else None, None)
            else:
                self.status = L.vrt_probe_gather(h, src.ctypes.data_as(C.POINTER(_ffi.Probe)) if a["inp"] else None, n, mv,
                                                 lc, pts, a["npoints"],
                                                 outs["sgs"].ctypes.data_as(C.POINTER(_ffi.SGRec)) if a["sgs"] else None,
                                                 vp("terms") if a["terms"] else None)
        self.error = L.vrt_last_error().decode(errors="replace")
        if dev:
            torch.cuda.synchronize()
            outs = {k: v.cpu().numpy() for k, v in d_out.items()}
        self.out = outs
        self.main = outs["sgs"] if name in GATHER else outs["rgb"]


def refused(call, status, text, what):
    assert call.status == status, (what, call.status, call.error)
    assert text in call.error, (what, call.error)
    assert not any(v.any() for v in call.out.values()), what  # nothing was written


# (case, keyword changes, entry points, status, piece of the message), in the order of the checks: null scene or
# n < 0, (n == 0: nothing to do), host-only scene, null pointers, the gather's point count, the cone step, the
# light map
T_C, ALL = TRACE + CONE, BATCH
REJECTED = [
    ("null scene", dict(scene=False), ALL, INVALID, "bad argument"),
    ("n < 0", dict(n=-1), ALL, INVALID, "bad argument"),
    ("null input", dict(inp=False), ALL, INVALID, "null argument"),
    ("null rgb", dict(rgb=False), T_C, INVALID, "null argument"),
    ("null light colour", dict(light=False), GATHER, INVALID, "null argument"),
    ("null sgs", dict(sgs=False), GATHER, INVALID, "null argument"),
    ("npoints 0", dict(points=True, npoints=0), GATHER, INVALID, "bad argument: 0 points (1..1024)"),
    ("npoints 1025", dict(points=True, npoints=1025), GATHER, INVALID, "bad argument: 1025 points (1..1024)"),
    ("infinite min_voxel", dict(min_voxel=math.inf), ALL, INVALID, "degenerate cone step"),
    # two at once: the earlier check answers
    ("null scene, n < 0", dict(scene=False, n=-1), ALL, INVALID, "bad argument"),
    ("null scene, n == 0", dict(scene=False, n=0), ALL, INVALID, "bad argument"),
    ("n < 0, null input", dict(n=-1, inp=False), ALL, INVALID, "bad argument"),
    ("null input, infinite min_voxel", dict(inp=False, min_voxel=math.inf), ALL, INVALID, "null argument"),
    ("null rgb, infinite min_voxel", dict(rgb=False, min_voxel=math.inf), T_C, INVALID, "null argument"),
    ("null sgs, bad npoints", dict(sgs=False, points=True, npoints=0), GATHER, INVALID, "null argument"),
    ("null light colour, bad npoints", dict(light=False, points=True, npoints=1025), GATHER, INVALID, "null argument"),
    ("bad npoints, infinite min_voxel", dict(points=True, npoints=1025, min_voxel=math.inf), GATHER, INVALID,
     "1025 points"),
]


@pytest.mark.parametrize("name", BATCH)
def test_batch_call_rejections(sc, name):
    for tree in (sc.tri, sc.probe):
        for case, kw, names, status, text in REJECTED:
            if name in names:
                refused(Call(sc, tree, name, **kw), status, text, case)


@pytest.mark.parametrize("name", BATCH)
def test_batch_calls_on_a_host_only_scene(sc, name):
    """n == 0 is nothing to do whatever the scene is and whatever else is
    passed; with work to do the host-only scene answers before the pointers,
    the point count and the cone step."""
    for kw in (dict(n=0), dict(n=0, inp=False, rgb=False, sgs=False, light=False),
               dict(n=0, points=True, npoints=0, min_voxel=math.inf)):
        c = Call(sc, sc.host_only, name, **kw)
        assert c.status == OK, (kw, c.error)
        assert not any(v.any() for v in c.out.values())
    refused(Call(sc, sc.host_only, name, n=-1), INVALID, "bad argument", "n < 0")
    for kw in (dict(), dict(inp=False), dict(rgb=False, sgs=False), dict(points=True, npoints=0),
               dict(min_voxel=math.inf), dict(inp=False, points=True, npoints=1025, min_voxel=math.inf)):
        refused(Call(sc, sc.host_only, name, **kw), NODEVICE, "host-only", kw)


@pytest.mark.parametrize("name", BATCH)
def test_batch_calls_need_a_light_map(sc, name):
    """The light map is asked for last: behind the pointers, the point count
    and the cone step."""
    for tree in (vrt.VoxelOctree(sc.sd, DEPTH), vrt.VoxelOctree(sc.sd, DEPTH, probes=sc.probes)):
        refused(Call(sc, tree, name), INVALID, "no light map", name)
        refused(Call(sc, tree, name, inp=False), INVALID, "null argument", name)
        refused(Call(sc, tree, name, min_voxel=math.inf), INVALID, "degenerate cone step", name)
        if name in GATHER:
            refused(Call(sc, tree, name, points=True, npoints=0), INVALID, "0 points", name)
            refused(Call(sc, tree, name, points=True, npoints=1025), INVALID, "1025 points", name)
            refused(Call(sc, tree, name, points=True), INVALID, "no light map", name)
        # n == 0 needs none
        assert Call(sc, tree, name, n=0).status == OK


@pytest.mark.parametrize("host,dev", [TRACE, CONE, GATHER])
def test_valid_batch_calls(sc, host, dev):
    """The valid call writes something, the host and the device forms agree
    bit for bit, and a min_voxel that is not > 0 (0, negative, NaN) is the
    scene's own."""
    for tree in (sc.tri, sc.probe):
        kw = dict(parts=True) if host in TRACE else dict(points=True, terms=True) if host in GATHER else {}
        a, b = Call(sc, tree, host, **kw), Call(sc, tree, dev, **kw)
        assert a.status == OK and b.status == OK, (a.error, b.error)
        assert a.main.any()
        for k in a.out:
            if host in TRACE and tree is sc.probe and k in ("rgb", "albedo"):
                continue  # the host form also shades the rays that end on a probe
            assert np.array_equal(pc.bits(a.out[k]), pc.bits(b.out[k])), (host, k)
        for mv in (-1.0, math.nan, tree.min_voxel(0)):
            c = Call(sc, tree, host, min_voxel=mv, **kw)
            assert c.status == OK, c.error
            assert all(np.array_equal(pc.bits(a.out[k]), pc.bits(c.out[k])) for k in a.out), mv
        if host in GATHER:  # the reference's own 100 points: npoints is not looked at
            c = Call(sc, tree, host, npoints=0)
            assert c.status == OK and c.main.any(), c.error
