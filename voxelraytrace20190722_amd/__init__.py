"""MI355X-native drop-in for jqly/VoxelRayTrace20190722's per-pixel
voxel-octree ray-march + ray/triangle hit loop.

The compute path is libvrt.so (HIP kernels for gfx950 behind the C ABI in
include/vrt.h); this package is its Python binding.  Importing the API loads
the library and raises if it is missing: there is no CPU fallback.
"""
from ._ffi import VrtError, lib, LIB_PATH  # noqa: F401
from .api import (  # noqa: F401
    FLT_MAX, Camera, Film, Light, MultiOctree, ObjModel, SceneData, VoxelOctree, multi_tile_map, build_id, build_flag, test_flags, device_count, device_selftest,
    device_selftest_order, device_selftest_chain,
    hdr_bytes, hdr_bytes_from_rgbe, intersect_triangle3, load_image, make_ray, obj2voxel, ray_march, ray_march_init, trace, cone_trace,
    TEST_FORCE_DEFER, TEST_FAIL_LAUNCH, TEST_SPILL_ALL, TEST_STREAM_LEFTOVER, TEST_LIGHT_TAIL, TEST_PRIM_TAIL, TEST_SEC_DEFER, TEST_SMALL_BATCH_CHUNK, TEST_SMALL_BEAM_ENTRY, TEST_UPDATE_TOO_LARGE, TEST_VIRTUAL_RANKS, render, set_test_flags, sweep_pose, tga_decode, tile_deal_map, tiles_per_rank, to_radian, tri_box_overlap,
    unpack_tiles_device, pack_tiles_c_device, unpack_tiles_c_device, write_hdr, rgbe_device, write_hdr_device,
    SG, LightProbe, probe_points, probe_eval, PROBE_SGS, PROBE_DIRS, TEST_SMALL_PROBE_CHUNK,
    probe_eval_device, expf_flavour, expf_model, expf_selftest,
    prod, inner_prod, sg_make, sg_integral, sg_prod, sg_inner_prod, sg_integral_device, sg_prod_device,
    sg_inner_prod_device, SG_COSINE_AMPLITUDE, SG_COSINE_SHARPNESS,
    digest, DIGEST_ITEMS, TEST_MULTI_REFUSE_LAST, TEST_MULTI_DIVERGE,
)

__all__ = [
    "VrtError", "lib", "LIB_PATH", "FLT_MAX", "Camera", "Film", "Light", "SceneData", "VoxelOctree", "MultiOctree",
    "multi_tile_map",
    "device_count", "device_selftest", "hdr_bytes", "intersect_triangle3", "make_ray",
    "ray_march", "ray_march_init", "trace", "cone_trace", "render", "sweep_pose", "tile_deal_map", "tiles_per_rank", "to_radian",
    "tri_box_overlap", "unpack_tiles_device", "pack_tiles_c_device", "unpack_tiles_c_device", "write_hdr", "ObjModel", "obj2voxel", "load_image",
    "tga_decode", "hdr_bytes_from_rgbe", "rgbe_device", "write_hdr_device", "build_id", "build_flag", "test_flags", "device_selftest_order", "set_test_flags",
    "device_selftest_chain", "SG", "LightProbe", "probe_points", "probe_eval",
    "probe_eval_device", "expf_flavour", "expf_model", "expf_selftest", "digest",
    "prod", "inner_prod", "sg_make", "sg_integral", "sg_prod", "sg_inner_prod", "sg_integral_device", "sg_prod_device",
    "sg_inner_prod_device", "SG_COSINE_AMPLITUDE", "SG_COSINE_SHARPNESS",
]
