"""The expf model on the host (vrt_expf_flavour, vrt_expf_model,
vrt_expf_selftest with device = -1) against this process's C library, and the
argument checks of the entry points of the device-shaded probe frames.  Bar:
bit-exact; no GPU."""
import ctypes as C

import numpy as np
import pytest

import voxelraytrace20190722_amd as vrt
from voxelraytrace20190722_amd import _ffi

f32 = np.float32
LO = int(f32(2.0 ** -27).view(np.uint32))   # bits(2^-27)
HI = int(f32(128.0).view(np.uint32))        # bits(128)
SIGN = 0x80000000
# the two inputs at which the flavours differ, with libm's (FMA) and the plain results
X_DIFF = [float.fromhex("0x1.04845ep+5"), float.fromhex("-0x1.f8cbb2p+5")]
Y_FUSED = [float.fromhex("0x1.f93e38p+46"), float.fromhex("0x1.f45326p-92")]
Y_PLAIN = [float.fromhex("0x1.f93e36p+46"), float.fromhex("0x1.f45324p-92")]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def nextf(x, up):
    return np.nextafter(f32(x), f32(np.inf if up else -np.inf), dtype=f32)


def edge_inputs():
    top, bot = f32(float.fromhex("0x1.62e42ep6")), f32(float.fromhex("-0x1.9fe368p6"))
    return np.array([0.0, -0.0, np.inf, -np.inf, np.finfo(f32).smallest_subnormal, 88.0, top, nextf(top, True),
                     bot, nextf(bot, True), nextf(bot, False), float.fromhex("-0x1.9d1d9ep6")], f32)


def libm_expf(x):
    """The C library's expf, one call per element (libm through ctypes: the
    function the library itself calls)."""
    m = C.CDLL("libm.so.6")
    m.expf.restype, m.expf.argtypes = C.c_float, [C.c_float]
    return np.array([m.expf(float(v)) for v in np.asarray(x, f32)], f32)


def test_flavour_is_known_and_fused_here():
    assert vrt.expf_flavour() in (0, 1)
    assert vrt.expf_flavour() == 1  # measured on this image: glibc's FMA variant


def test_host_model_equals_libm_on_every_pattern_of_the_working_range():
    """Every bit pattern with |x| in [2^-27, 128), both signs: 2 x 285,212,672."""
    f = vrt.expf_flavour()
    for first in (LO, LO | SIGN):
        bad, where = vrt.expf_selftest(first, HI - LO, 1, f, device=-1)
        assert bad == 0, f"{bad} mismatches, first at bits {where:#x}"


def test_host_model_equals_libm_over_the_whole_space_at_stride_61():
    bad, where = vrt.expf_selftest(0, (2 ** 32 + 60) // 61, 61, vrt.expf_flavour(), device=-1)
    assert bad == 0, f"{bad} mismatches, first at bits {where}"


def test_the_selftest_sees_the_other_flavour_differ():
    """The positive input at which the flavours differ lies in the working
    range: the other flavour's sweep reports exactly it."""
    f = vrt.expf_flavour()
    bad, where = vrt.expf_selftest(LO, HI - LO, 1, 1 - f, device=-1)
    assert (bad, where) == (1, int(bits([X_DIFF[0]])[0]))
    # wrap-around and NaN skipping: a sweep across the top of the space
    bad, _ = vrt.expf_selftest(0xFFFFFF00, 0x200, 1, f, device=-1)
    assert bad == 0


def test_the_two_flavours_at_the_inputs_where_they_differ():
    assert np.array_equal(bits(vrt.expf_model(X_DIFF, 0)), bits(Y_PLAIN))
    assert np.array_equal(bits(vrt.expf_model(X_DIFF, 1)), bits(Y_FUSED))


def test_pinned_edges_equal_libm():
    x = edge_inputs()
    want = libm_expf(x)
    assert np.array_equal(bits(vrt.expf_model(x, vrt.expf_flavour())), bits(want))
    # both flavours agree there, and the special cases are the documented ones
    assert np.array_equal(bits(vrt.expf_model(x, 0)), bits(vrt.expf_model(x, 1)))
    got = vrt.expf_model(x, 1)
    assert got[0] == 1 and got[1] == 1 and got[2] == np.inf and bits(got[3:4])[0] == 0
    assert np.isfinite(got[6]) and got[7] == np.inf       # 0x1.62e42ep6 and its successor
    assert got[8] > 0 and bits(got[10:11])[0] == 0        # -0x1.9fe368p6 and the float below it


def test_nan_in_nan_out():
    x = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], np.uint32).view(f32)
    for f in (0, 1):
        assert np.isnan(vrt.expf_model(x, f)).all()


def test_argument_checks():
    L = vrt.lib()
    inv = _ffi.VRT_E_INVALID
    x = np.zeros(4, f32)
    px = x.ctypes.data_as(_ffi.f32p)
    bad, first, fl = C.c_uint64(), C.c_uint32(), C.c_int()
    assert L.vrt_expf_flavour(None) == inv
    assert L.vrt_expf_flavour(C.byref(fl)) == _ffi.VRT_OK
    assert L.vrt_expf_model(None, 4, 1, px) == inv
    assert L.vrt_expf_model(px, 4, 1, None) == inv
    assert L.vrt_expf_model(px, -1, 1, px) == inv
    assert L.vrt_expf_model(px, 4, 2, px) == inv and L.vrt_expf_model(px, 4, -1, px) == inv
    assert L.vrt_expf_model(None, 0, 0, None) == _ffi.VRT_OK
    assert L.vrt_expf_selftest(-1, 0, 16, 1, 1, None, C.byref(first)) == inv
    assert L.vrt_expf_selftest(-1, 0, 16, 1, 2, C.byref(bad), C.byref(first)) == inv
    assert L.vrt_expf_selftest(-1, 0, 16, 1, 1, C.byref(bad), None) == _ffi.VRT_OK and bad.value == 0
    # device arrays: checked before any device is touched
    one = C.c_void_p(64)
    assert L.vrt_probe_eval_device(0, None, 1, one, 1, one, None) == inv
    assert L.vrt_probe_eval_device(0, one, 1, None, 1, one, None) == inv
    assert L.vrt_probe_eval_device(0, one, 1, one, 1, None, None) == inv
    assert L.vrt_probe_eval_device(0, one, -1, one, 1, one, None) == inv
    assert L.vrt_probe_eval_device(0, one, 1, one, -1, one, None) == inv
    # the scene calls with a NULL scene
    cam = vrt.Camera(vrt.to_radian(60), (0, 0, 3), (0, 0, 0), (0, 1, 0))
    film = vrt.Film(1, 1, 8, 8)
    hits = C.c_int64()
    assert L.vrt_probe_shade_hits_device(None, one, 1, one, one, None) == inv
    assert L.vrt_render_trace_probes(None, C.byref(cam.c), C.byref(film.c), 0.0, px, None, None) == inv
    assert L.vrt_render_trace_probes_device(None, C.byref(cam.c), C.byref(film.c), 0.0, 0, 1, 1, one, None) == inv
    assert L.vrt_trace_frame_probes_device(None, C.byref(cam.c), C.byref(film.c), None, C.byref(cam.c),
                                           C.byref(film.c), 0.0, 0, 1, 1, one, None, C.byref(hits)) == inv
