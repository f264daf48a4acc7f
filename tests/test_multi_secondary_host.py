"""Config 5 on the multi-device handle, host side: the three new symbols
(vrt_render_secondary_tiles_device, vrt_render_secondary_multi[_device]), their
ctypes signatures and what they answer before a device is looked at.  No
device is needed: a NULL handle, NULL arguments and a bad spp are refused
first, and a host-only scene answers VRT_E_NODEVICE as every device call
does."""
import ctypes as C

import numpy as np
import pytest

import voxelraytrace20190722_amd as vrt
from voxelraytrace20190722_amd import _ffi

_P = C.c_void_p
CAMP, FILMP = C.POINTER(_ffi.Camera), C.POINTER(_ffi.Film)
WANT = {
    "vrt_render_secondary_tiles_device": [_P, CAMP, FILMP, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P],
    "vrt_render_secondary_multi": [_P, CAMP, FILMP, C.c_int, _ffi.f32p, _ffi.i64p],
    "vrt_render_secondary_multi_device": [_P, CAMP, FILMP, C.c_int, _P, _P],
}
INV, NODEV = _ffi.VRT_E_INVALID, _ffi.VRT_E_NODEVICE


def _view():
    cam = vrt.Camera(vrt.to_radian(60), (1, 10, 1), (0, 0, 0), (0, 1, 0))
    film = vrt.Film(1, 1, 16, 16)
    return cam, film, C.byref(cam.c), C.byref(film.c)


def test_symbols_resolve_with_their_signatures():
    L = vrt.lib()
    for name, args in WANT.items():
        assert name in _ffi.SIGNATURES, name
        res, got = _ffi.SIGNATURES[name]
        assert res is C.c_int and got == args, name
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args, name
    assert hasattr(vrt.VoxelOctree, "render_secondary_tiles_device")
    for name in ("render_secondary", "render_secondary_device"):
        assert hasattr(vrt.MultiOctree, name), name


def test_null_handle_arguments_and_spp():
    L = vrt.lib()
    _, _, c, f = _view()
    vis = np.full((16, 16), 7.0, np.float32)
    p, d = vis.ctypes.data_as(_ffi.f32p), C.c_void_p(vis.ctypes.data)
    rays = C.c_int64(-7)
    # a NULL handle, whatever else is passed (no handle exists without a device)
    for spp in (0, 1, 64, 65):
        assert L.vrt_render_secondary_multi(None, c, f, spp, p, C.byref(rays)) == INV
        assert L.vrt_render_secondary_multi_device(None, c, f, spp, d, None) == INV
    assert L.vrt_render_secondary_multi(None, None, None, 64, None, None) == INV
    assert L.vrt_render_secondary_multi_device(None, None, None, 64, None, None) == INV
    assert b"null" in L.vrt_last_error()
    # the single-scene call without a scene
    for spp in (0, 64, 65):
        assert L.vrt_render_secondary_tiles_device(None, c, f, spp, 0, 1, d, d, d, None, None) == INV
    assert rays.value == -7 and np.all(vis == 7.0)


def test_host_only_scene_has_no_device():
    """device < 0: VRT_E_NODEVICE from the single-scene call, before its other
    arguments are looked at (as vrt_render_secondary_device answers)."""
    L = vrt.lib()
    cam, film, c, f = _view()
    tree = vrt.VoxelOctree(vrt.SceneData.proxy(0.05, 2), 3, device=-1)
    buf = np.zeros(16 * 16 * 8, np.float32)
    d = C.c_void_p(buf.ctypes.data)
    assert L.vrt_render_secondary_tiles_device(tree.h, c, f, 64, 0, 1, d, d, d, None, None) == NODEV
    assert L.vrt_render_secondary_device(tree.h, c, f, 64, 0, 1, d, d, None) == NODEV
    for spp in (0, 65):
        assert L.vrt_render_secondary_tiles_device(tree.h, c, f, spp, 0, 1, d, d, d, None, None) == NODEV
    with pytest.raises(vrt.VrtError) as e:
        tree.render_secondary_tiles_device(cam, film, 64, 0, 1, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data)
    assert e.value.status == NODEV
    assert not buf.any()
