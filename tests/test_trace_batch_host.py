"""Batched trace() / cone_trace (vrt_trace_batch, vrt_cone_trace_batch): what
can be checked without a device -- the exported symbols and their ctypes
prototypes, the host-only scene's error, the empty batch and the shape
checks of the Python binding."""
import ctypes as C

import numpy as np
import pytest

import voxelraytrace20190722_amd as vrt
from voxelraytrace20190722_amd import _ffi

SYMBOLS = ("vrt_trace_batch", "vrt_trace_batch_device", "vrt_cone_trace_batch", "vrt_cone_trace_batch_device")


@pytest.fixture(scope="module")
def host_tree():
    return vrt.VoxelOctree(vrt.SceneData.proxy(0.05, 2), 3, device=-1)


def test_symbols_exported():
    L = C.CDLL(vrt.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(L, name), name
    for name in ("trace", "cone_trace"):
        assert name in vrt.__all__ and callable(getattr(vrt, name)), name
    for name in ("trace", "cone_trace", "trace_device", "cone_trace_device"):
        assert callable(getattr(vrt.VoxelOctree, name)), name
    assert vrt.TEST_SMALL_BATCH_CHUNK == 0x10000


def test_ffi_prototypes_load():
    L = vrt.lib()
    for name in SYMBOLS:
        res, args = _ffi.SIGNATURES[name]
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert C.sizeof(_ffi.ISect) == 24
    assert C.sizeof(_ffi.TraceParts) == 4 * C.sizeof(C.c_void_p)


def test_host_only_scene_has_no_device(host_tree):
    rays = np.zeros((3, 8), np.float32)
    rays[:, 5] = 1.0
    with pytest.raises(vrt.VrtError) as e:
        host_tree.trace(rays)
    assert e.value.status == _ffi.VRT_E_NODEVICE
    with pytest.raises(vrt.VrtError) as e:
        vrt.trace(host_tree, rays, parts=True)
    assert e.value.status == _ffi.VRT_E_NODEVICE
    with pytest.raises(vrt.VrtError) as e:
        host_tree.cone_trace(np.zeros((2, 3), np.float32), np.ones((2, 3), np.float32))
    assert e.value.status == _ffi.VRT_E_NODEVICE
    with pytest.raises(vrt.VrtError) as e:
        vrt.cone_trace(host_tree, np.zeros((2, 3), np.float32), np.ones((2, 3), np.float32))
    assert e.value.status == _ffi.VRT_E_NODEVICE


def test_empty_batch_needs_no_device(host_tree):
    rgb = host_tree.trace(np.zeros((0, 8), np.float32))
    assert rgb.shape == (0, 3) and rgb.dtype == np.float32
    rgb, parts = host_tree.trace(np.zeros((0, 8), np.float32), parts=True)
    assert rgb.shape == (0, 3)
    assert sorted(parts) == ["albedo", "direct", "hit", "hit_p", "indirect", "normal", "tri", "voxel"]
    for key in ("hit", "tri", "voxel"):
        assert parts[key].shape == (0,), key
    for key in ("hit_p", "normal", "indirect", "direct", "albedo"):
        assert parts[key].shape == (0, 3), key
    out = host_tree.cone_trace(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    assert out.shape == (0, 3) and out.dtype == np.float32
    # the raw calls: n == 0 touches nothing, n < 0 is an argument error
    L = vrt.lib()
    assert L.vrt_trace_batch(host_tree.h, None, 0, 0.0, None, None) == _ffi.VRT_OK
    assert L.vrt_cone_trace_batch(host_tree.h, None, 0, 0.0, None) == _ffi.VRT_OK
    assert L.vrt_trace_batch_device(host_tree.h, None, 0, 0.0, None, None, None) == _ffi.VRT_OK
    assert L.vrt_cone_trace_batch_device(host_tree.h, None, 0, 0.0, None, None) == _ffi.VRT_OK
    assert L.vrt_trace_batch(host_tree.h, None, -1, 0.0, None, None) == _ffi.VRT_E_INVALID
    assert L.vrt_cone_trace_batch(host_tree.h, None, -1, 0.0, None) == _ffi.VRT_E_INVALID
    assert L.vrt_trace_batch(None, None, 0, 0.0, None, None) == _ffi.VRT_E_INVALID


@pytest.mark.parametrize("shape", [(8,), (4, 7), (2, 2, 8), (0,)])
def test_trace_rejects_malformed_rays(host_tree, shape):
    with pytest.raises(ValueError):
        host_tree.trace(np.zeros(shape, np.float32))


@pytest.mark.parametrize("ps,ns", [((3,), (3,)), ((4, 3), (5, 3)), ((4, 2), (4, 2)), ((4, 3), (4, 6))])
def test_cone_trace_rejects_malformed_points(host_tree, ps, ns):
    with pytest.raises(ValueError):
        host_tree.cone_trace(np.zeros(ps, np.float32), np.zeros(ns, np.float32))
