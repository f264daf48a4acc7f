"""The SG algebra on the host: vrt_sg_make, vrt_sg_integral, vrt_sg_prod and
vrt_sg_inner_prod against reference_gi_cases.sg_model, the float32 restatement
that tests/test_reference_gi_host.py::test_sg_algebra pins to the reference's
compiled code, and, where oracle/_ref/libvrtref_gi.so is built, against that
code directly (rgi_sg_ops, rgi_sg_make of oracle/ref_gi_glue.cc).

Bar: identity -- every float equal in its bits, NaN matching NaN; no
tolerance.  No GPU is used."""
import ctypes as C

import numpy as np
import pytest

import pyoracle as po
import voxelraytrace20190722_amd as vrt
from voxelraytrace20190722_amd import _ffi

import reference_gi_cases as rc

F = np.float32


@pytest.fixture(scope="module")
def live():
    if not po.reference_gi_available():
        if po.reference_sources_present():
            pytest.fail("the reference sources are present but oracle/_ref/libvrtref_gi.so was not built "
                        "(oracle/Makefile)")
        pytest.skip("reference sources absent: oracle/_ref/libvrtref_gi.so cannot be built")
    return po.reference_gi()


@pytest.fixture(scope="module")
def pairs():
    return rc.sg_pairs(12, 512)


@pytest.fixture(scope="module")
def model(pairs):
    return rc.sg_model(*pairs)


def make_inputs(pairs):
    """Constructor inputs: the pairs' amplitudes and sharpnesses with axes that
    are not unit -- scaled, tiny, huge (d.d overflows), zero and NaN."""
    lhs, rhs, dirs = pairs
    a, s = lhs[:, 0:3].copy(), lhs[:, 6].copy()
    d = (rhs[:, 3:6] * np.random.default_rng(5).uniform(0.1, 9.0, (len(rhs), 1))).astype(F)
    d[0] = 0.0
    d[1] = (1e-30, 2e-30, -1e-30)
    d[2] = (3e25, 1e20, -2e24)
    d[3, 1] = np.nan
    d[4] = (0.0, -0.0, 5.0)
    return a, np.ascontiguousarray(d), s


def ref_sg_make(L, a, d, s):
    """gi::SG{a, d, s} of the reference, one record at a time."""
    out = np.zeros((len(a), 7), F)
    f32p = C.POINTER(C.c_float)
    for i in range(len(a)):
        ai, di = np.ascontiguousarray(a[i]), np.ascontiguousarray(d[i])
        L.rgi_sg_make(ai.ctypes.data_as(f32p), di.ctypes.data_as(f32p), float(s[i]),
                      out[i].ctypes.data_as(f32p))
    return out


def test_host_calls_equal_the_model(pairs, model):
    lhs, rhs, _ = pairs
    integral, prod, inner = vrt.sg_integral(lhs), vrt.sg_prod(lhs, rhs), vrt.sg_inner_prod(lhs, rhs)
    assert rc.same_f32(integral, model["integral"]), rc.diff_count(integral, model["integral"])
    assert rc.same_f32(prod, model["prod"]), rc.diff_count(prod, model["prod"])
    assert rc.same_f32(inner, model["inner"]), rc.diff_count(inner, model["inner"])
    # the set tests both: sharpness 0 gives inf * 0, most rows are finite
    assert np.isnan(integral).any() and np.isfinite(integral).all(axis=1).sum() > 300
    assert np.isnan(inner).any() and np.isfinite(inner).all(axis=1).sum() > 300
    # unnormalised results went through the constructor
    assert (np.abs(np.linalg.norm(model["prod"][:, 3:6].astype(np.float64), axis=1) - 1) < 1e-6).sum() > 300


def test_host_calls_equal_the_reference(live, pairs):
    lhs, rhs, dirs = pairs
    _, integral, prod, inner = po.ref_sg_ops(lhs, rhs, dirs)
    assert rc.same_f32(vrt.sg_integral(lhs), integral)
    assert rc.same_f32(vrt.sg_prod(lhs, rhs), prod)
    assert rc.same_f32(vrt.sg_inner_prod(lhs, rhs), inner)


def test_sg_make_normalises_as_the_constructor(pairs):
    a, d, s = make_inputs(pairs)
    got = vrt.sg_make(a, d, s)
    with np.errstate(all="ignore"):
        want = np.concatenate([a, (d / np.sqrt(rc._dot(d, d))[:, None]).astype(F), s[:, None]], axis=1)
    assert rc.same_f32(got, want), rc.diff_count(got, want)
    assert np.isnan(got[0, 3:6]).all() and np.isnan(got[3, 3:6]).all()  # zero and NaN axes
    assert not got[2, 3:6].any()  # d.d overflows: x / inf = 0
    assert np.isfinite(got[5:]).all()


def test_sg_make_equals_the_reference(live, pairs):
    a, d, s = make_inputs(pairs)
    assert rc.same_f32(vrt.sg_make(a, d, s), ref_sg_make(live, a, d, s))


def test_objects_under_the_reference_names(pairs, model):
    lhs, rhs, _ = pairs
    for i in (0, 7, 100, 511):
        l, r = vrt.SG(lhs[i, 0:3], lhs[i, 3:6], lhs[i, 6]), vrt.SG(rhs[i, 0:3], rhs[i, 3:6], rhs[i, 6])
        assert rc.same_f32(l.integral(), model["integral"][i])
        p = vrt.prod(l, r)
        assert rc.same_f32(np.concatenate([p.a, p.d, [p.s]]), model["prod"][i])
        assert rc.same_f32(vrt.inner_prod(l, r), model["inner"][i])
    g = vrt.SG.make((1, 2, 3), (0, 3, 4), 10)
    assert rc.same_f32(np.concatenate([g.a, g.d, [g.s]]),
                       np.array([1, 2, 3, 0, F(3) / F(5), F(4) / F(5), 10], F))


def test_n_zero_and_one(pairs, model):
    lhs, rhs, _ = pairs
    e7, e3 = np.zeros((0, 7), F), np.zeros((0, 3), F)
    assert vrt.sg_integral(e7).shape == (0, 3) and vrt.sg_prod(e7, e7).shape == (0, 7)
    assert vrt.sg_inner_prod(e7, e7).shape == (0, 3) and vrt.sg_make(e3, e3, np.zeros(0, F)).shape == (0, 7)
    # n == 0 touches nothing and asks for no array
    L = vrt.lib()
    assert L.vrt_sg_integral(None, 0, None) == 0 and L.vrt_sg_prod(None, None, 0, None) == 0
    assert L.vrt_sg_inner_prod(None, None, 0, None) == 0 and L.vrt_sg_make(None, None, None, 0, None) == 0
    assert rc.same_f32(vrt.sg_integral(lhs[9:10]), model["integral"][9:10])
    assert rc.same_f32(vrt.sg_prod(lhs[9:10], rhs[9:10]), model["prod"][9:10])
    assert rc.same_f32(vrt.sg_inner_prod(lhs[9:10], rhs[9:10]), model["inner"][9:10])


def test_null_and_negative_arguments_are_refused(pairs):
    lhs, rhs, _ = pairs
    L = vrt.lib()
    sg = lambda a: a.ctypes.data_as(C.POINTER(_ffi.SGRec))
    fp = lambda a: a.ctypes.data_as(_ffi.f32p)
    l, r = np.ascontiguousarray(lhs[:4]), np.ascontiguousarray(rhs[:4])
    o3, o7 = np.full((4, 3), 7, F), np.full((4, 7), 7, F)
    a, d, s = np.ones((4, 3), F), np.ones((4, 3), F), np.ones(4, F)
    calls = [
        lambda: L.vrt_sg_integral(None, 4, fp(o3)), lambda: L.vrt_sg_integral(sg(l), 4, None),
        lambda: L.vrt_sg_integral(sg(l), -1, fp(o3)),
        lambda: L.vrt_sg_prod(None, sg(r), 4, sg(o7)), lambda: L.vrt_sg_prod(sg(l), None, 4, sg(o7)),
        lambda: L.vrt_sg_prod(sg(l), sg(r), 4, None), lambda: L.vrt_sg_prod(sg(l), sg(r), -1, sg(o7)),
        lambda: L.vrt_sg_inner_prod(None, sg(r), 4, fp(o3)), lambda: L.vrt_sg_inner_prod(sg(l), None, 4, fp(o3)),
        lambda: L.vrt_sg_inner_prod(sg(l), sg(r), 4, None), lambda: L.vrt_sg_inner_prod(sg(l), sg(r), -1, fp(o3)),
        lambda: L.vrt_sg_make(None, fp(d), fp(s), 4, sg(o7)), lambda: L.vrt_sg_make(fp(a), None, fp(s), 4, sg(o7)),
        lambda: L.vrt_sg_make(fp(a), fp(d), None, 4, sg(o7)), lambda: L.vrt_sg_make(fp(a), fp(d), fp(s), 4, None),
        lambda: L.vrt_sg_make(fp(a), fp(d), fp(s), -1, sg(o7)),
    ]
    for k, call in enumerate(calls):
        assert call() == _ffi.VRT_E_INVALID, k
    assert np.all(o3 == 7) and np.all(o7 == 7)  # a refused call writes nothing
