"""Several lights in one light map (vrt_lightmap_build_lights and the frame
and multi-device calls over a light list): what can be checked without a
device -- the exported symbols, the ctypes layout of vrt_light against the
library's own sizeof, the host-only scene's error and the Python classes."""
import ctypes as C

import pytest

import voxelraytrace20190722_amd as vrt
from voxelraytrace20190722_amd import _ffi, api

SYMBOLS = ("vrt_lightmap_build_lights", "vrt_trace_frame_lights_device", "vrt_lightmap_build_lights_multi",
           "vrt_trace_frame_lights_multi", "vrt_trace_frame_lights_multi_device")


@pytest.fixture(scope="module")
def host_tree():
    return vrt.VoxelOctree(vrt.SceneData.proxy(0.05, 2), 3, device=-1)


def lights(n, film=(64, 64)):
    cam = vrt.Camera(vrt.to_radian(60), (1.0, 10.0, 1.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    return [vrt.Light(cam, vrt.Film(1, 1, *film), (1.0, 0.5 + 0.03 * i, 0.25)) for i in range(n)]


def test_symbols_exported_and_prototypes_load():
    raw = C.CDLL(vrt.LIB_PATH)
    L = vrt.lib()
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        res, args = _ffi.SIGNATURES[name]
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert "Light" in vrt.__all__
    for name in ("lightmap_lights", "trace_frame_lights_device"):
        assert callable(getattr(vrt.VoxelOctree, name)), name
    for name in ("lightmap_lights", "trace_frame_lights", "trace_frame_lights_device"):
        assert callable(getattr(vrt.MultiOctree, name)), name


def test_vrt_light_layout():
    assert C.sizeof(_ffi.LightRec) == vrt.build_flag("VRT_SIZEOF_LIGHT")
    assert C.sizeof(_ffi.LightRec) == C.sizeof(_ffi.Camera) + C.sizeof(_ffi.Film) + 12
    assert _ffi.LightRec.film.offset == C.sizeof(_ffi.Camera)
    assert _ffi.LightRec.color.offset == C.sizeof(_ffi.Camera) + C.sizeof(_ffi.Film)
    assert vrt.build_flag("VRT_MAX_LIGHTS") == 16


def test_light_list_argument():
    ls = lights(3)
    arr, n = api._lights_arg(ls)
    assert n == 3 and len(arr) == 3
    for i, l in enumerate(ls):
        assert list(arr[i].color) == [float(v) for v in l.color]
        assert (arr[i].film.nx, arr[i].film.ny) == (64, 64)
        assert bytes(arr[i].cam) == bytes(l.camera.c)
    assert list(vrt.Light(ls[0].camera, ls[0].film).color) == [1.0, 1.0, 1.0]
    assert api._lights_arg(None) == (None, 0)
    assert api._lights_arg([])[1] == 0


def test_host_only_scene_has_no_device(host_tree):
    with pytest.raises(vrt.VrtError) as e:
        host_tree.lightmap_lights(lights(2))
    assert e.value.status == _ffi.VRT_E_NODEVICE
    view, film = lights(1)[0].camera, vrt.Film(1, 1, 40, 32)
    with pytest.raises(vrt.VrtError) as e:
        host_tree.trace_frame_lights_device(lights(2), view, film, 0, 1, 1, None)
    assert e.value.status == _ffi.VRT_E_NODEVICE
    # the device comes first, as in vrt_lightmap_build: also with a bad list
    L = vrt.lib()
    assert L.vrt_lightmap_build_lights(host_tree.h, None, 0, None) == _ffi.VRT_E_NODEVICE
    assert L.vrt_lightmap_build_lights(None, None, 0, None) == _ffi.VRT_E_INVALID
    assert L.vrt_lightmap_build_lights_multi(None, None, 0, None) == _ffi.VRT_E_INVALID
