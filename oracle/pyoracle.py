"""TEST INFRASTRUCTURE ONLY: ctypes binding of oracle/liboracle.so (the CPU
restatement, vrt_oracle.c) and of oracle/_ref/libvrtref.so (the reference's
own raytri.cc / tribox2.cc / stb_image_write.h, compiled unmodified) and
oracle/_ref/libvrtref_gi.so (the reference's own camera.cc and voxel_octree.cc,
compiled unmodified, behind oracle/ref_gi_glue.cc).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import
this module; the product (libvrt.so, voxelraytrace20190722_amd) never does.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_SO = os.path.join(HERE, "liboracle.so")
REF_SO = os.path.join(HERE, "_ref", "libvrtref.so")
REF_GI_SO = os.path.join(HERE, "_ref", "libvrtref_gi.so")

f32p = C.POINTER(C.c_float)
f64p = C.POINTER(C.c_double)
i32p = C.POINTER(C.c_int32)
u32p = C.POINTER(C.c_uint32)
i64p = C.POINTER(C.c_int64)
u8p = C.POINTER(C.c_uint8)
P = C.c_void_p

_o = None
_r = None
_g = None


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def oracle():
    global _o
    if _o is None:
        if not os.path.exists(ORACLE_SO):
            raise ImportError(f"{ORACLE_SO} missing: run `make -C oracle`")
        L = C.CDLL(ORACLE_SO)
        sig = {
            "ora_intersect_triangle3": (C.c_int, [f64p] * 8),
            "ora_tri_box_overlap": (C.c_int, [f32p, f32p, f32p]),
            "ora_camera_init": (None, [C.c_float, f32p, f32p, f32p, C.c_float, C.c_float, f32p]),
            "ora_gen_rays4": (C.c_int, [f32p, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, f32p]),
            "ora_gen_rays1": (C.c_int, [f32p, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, f32p]),
            "ora_make_ray": (None, [f32p, f32p, C.c_float, C.c_float, f32p]),
            "ora_aabb_isect": (C.c_int, [f32p, f32p]),
            "ora_sort8": (None, [f32p, i32p]),
            "ora_first_min": (C.c_int, [f32p, C.c_int]),
            "ora_scene_create": (P, [f32p, f32p, f32p, i32p, C.c_int, C.c_int]),
            "ora_scene_set_materials": (None, [P, C.c_int, i32p, f32p, C.c_int, i32p, i64p, u8p, C.c_int64]),
            "ora_scene_destroy": (None, [P]),
            "ora_scene_info": (None, [P, i64p, f32p]),
            "ora_scene_boxes": (None, [P, C.POINTER(C.c_uint64), f32p]),
            "ora_scene_leaves": (None, [P, u32p, u32p, i32p]),
            "ora_ray_march": (None, [P, f32p, C.c_int, i32p, i32p, u32p, f32p, f32p, u32p]),
            "ora_shade": (None, [P, f32p, C.c_int, f32p]),
            "ora_render": (None, [P, f32p, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int,
                                  f32p, i32p, i32p, u32p, f32p, u32p]),
            "ora_render_rows": (C.c_double, [P, f32p, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int,
                                             C.c_int, C.c_int, f32p]),
            "ora_linear_to_rgbe": (None, [f32p, u8p]),
            "ora_pcg_next": (C.c_uint32, [C.POINTER(C.c_uint64)]),
            "ora_uniform_m11": (C.c_float, [C.POINTER(C.c_uint64)]),
            "ora_random_point_in_unit_sphere": (None, [C.POINTER(C.c_uint64), f32p]),
            "ora_render_secondary": (C.c_int64, [P, f32p, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int,
                                                 C.c_int, f32p, i32p, i32p, u32p]),
            "ora_lightmap": (C.c_int64, [P, f32p, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int]),
            "ora_lightmap_filter": (None, [P]),
            "ora_lightmap_nodes": (None, [P, C.POINTER(C.c_uint64), f32p, f32p]),
            "ora_min_voxel": (C.c_float, [P, C.c_int]),
            "ora_cone_trace": (None, [P, f32p, C.c_int, C.c_float, f32p]),
            "ora_hit_pieces": (None, [P, f32p, C.c_int, f32p, f32p, f32p]),
            "ora_travorder": (None, [f32p, f32p, i32p, f32p]),
            "ora_shade_trace": (None, [P, f32p, C.c_int, C.c_float, f32p]),
            "ora_render_trace": (None, [P, f32p, C.c_float, C.c_float, C.c_int, C.c_int, C.c_float, C.c_int,
                                        f32p, i32p, f32p]),
        }
        for k, (res, args) in sig.items():
            f = getattr(L, k)
            f.restype = res
            f.argtypes = args
        _o = L
    return _o


def sort8(dist):
    """travorder's std::sort of the 8 Items by dist -> child order (8,)."""
    d = np.ascontiguousarray(np.asarray(dist, np.float32).reshape(8))
    o = np.zeros(8, np.int32)
    oracle().ora_sort8(_p(d, f32p), _p(o, i32p))
    return o


def travorder(box, ray):
    """travorder on split()'s children of `box` -> (order (8,), child boxes (8, 6))."""
    box = np.ascontiguousarray(np.asarray(box, np.float32).reshape(6))
    ray = np.ascontiguousarray(np.asarray(ray, np.float32).reshape(8))
    o = np.zeros(8, np.int32)
    child = np.zeros((8, 6), np.float32)
    oracle().ora_travorder(_p(box, f32p), _p(ray, f32p), _p(o, i32p), _p(child, f32p))
    return o, child


def first_min(depth):
    """ray_march_isect's std::min_element index (-1 if empty)."""
    d = np.ascontiguousarray(np.asarray(depth, np.float32).reshape(-1))
    return int(oracle().ora_first_min(_p(d, f32p), d.shape[0]))


def reference_available():
    return os.path.exists(REF_SO)


def reference():
    """The reference's own primitives (oracle/_ref/libvrtref.so)."""
    global _r
    if _r is None:
        if not os.path.exists(REF_SO):
            raise ImportError(f"{REF_SO} missing (built only where /root/reference exists)")
        L = C.CDLL(REF_SO)
        L.ref_intersect_triangle3.restype = C.c_int
        L.ref_intersect_triangle3.argtypes = [f64p] * 6 + [C.POINTER(C.c_int)]
        L.ref_tri_box_overlap.restype = C.c_int
        L.ref_tri_box_overlap.argtypes = [f32p, f32p, f32p]
        L.ref_write_hdr_mem.restype = C.c_long
        L.ref_write_hdr_mem.argtypes = [C.c_int, C.c_int, C.c_int, f32p, u8p, C.c_long]
        L.ref_load_obj.restype = C.POINTER(_RefObj)
        L.ref_load_obj.argtypes = [C.c_char_p, C.c_char_p]
        L.ref_free_obj.restype = None
        L.ref_free_obj.argtypes = [C.POINTER(_RefObj)]
        L.ref_stbi_load.restype = u8p
        L.ref_stbi_load.argtypes = [C.c_char_p, i32p, i32p, i32p]
        L.ref_stbi_load_mem.restype = u8p
        L.ref_stbi_load_mem.argtypes = [u8p, C.c_int, i32p, i32p, i32p]
        L.ref_stbi_free.restype = None
        L.ref_stbi_free.argtypes = [u8p]
        L.ref_stbi_failure.restype = C.c_char_p
        _r = L
    return _r


# oracle/Makefile's REF
REF_SRC = os.environ.get("REF", "/root/reference/VoxelRayTrace20190722")


def reference_sources_present():
    """The reference's own sources, from which oracle/Makefile builds _ref/."""
    return os.path.exists(os.path.join(REF_SRC, "voxel_octree.cc"))


def reference_gi_available():
    return os.path.exists(REF_GI_SO)


def reference_gi():
    """The reference's own camera, octree, march, light map, cone trace and
    light probes (oracle/_ref/libvrtref_gi.so)."""
    global _g
    if _g is None:
        if not os.path.exists(REF_GI_SO):
            raise ImportError(f"{REF_GI_SO} missing (built only where the reference sources and clang++ exist)")
        L = C.CDLL(REF_GI_SO)
        u64p = C.POINTER(C.c_uint64)
        sig = {
            "rgi_scene_create": (P, [f32p, f32p, f32p, i32p, C.c_int, C.c_int, f32p, C.POINTER(C.c_char_p), f32p,
                                     C.c_int, C.c_int]),
            "rgi_scene_destroy": (None, [P]),
            "rgi_tree_info": (None, [P, i64p]),
            "rgi_tree_dump": (None, [P, u64p, i32p, f32p, f32p, f32p, i32p, i32p]),
            "rgi_gen_rays": (None, [f32p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, f32p]),
            "rgi_make_ray": (None, [f32p, f32p, C.c_float, C.c_float, f32p]),
            "rgi_aabb_isect": (None, [f32p, f32p, C.c_int, i32p]),
            "rgi_travorder": (None, [f32p, f32p, C.c_int, i32p, f32p]),
            "rgi_ray_march": (None, [P, f32p, C.c_int, C.c_int, f32p, i32p, i32p, u32p, f32p, f32p, f32p, f32p, i32p,
                                     f32p]),
            "rgi_lightmap": (C.c_int64, [P, f32p, C.c_float, C.c_float, C.c_int, C.c_int, f32p]),
            "rgi_lightmap_filter": (None, [P]),
            "rgi_min_voxel": (C.c_float, [P, C.c_int]),
            "rgi_cone_trace": (None, [P, f32p, C.c_int, C.c_float, f32p]),
            "rgi_film_add": (None, [C.c_float, C.c_float, C.c_int, C.c_int, i32p, f32p, C.c_int, f32p]),
            "rgi_probe_isect": (None, [f32p, f32p, f32p, C.c_int, i32p, f32p]),
            "rgi_probe_overlap": (None, [f32p, f32p, C.c_int, i32p]),
            "rgi_probe_gather": (None, [P, f32p, C.c_int, C.c_float, f32p, f32p, f32p]),
            "rgi_scene_probe_gather": (None, [P, C.c_int, C.c_float, f32p, f32p, f32p]),
            "rgi_probe_eval": (None, [f32p, f32p, C.c_int, f32p]),
            "rgi_sg_ops": (None, [f32p, f32p, f32p, C.c_int, f32p, f32p, f32p, f32p]),
            "rgi_sg_make": (None, [f32p, f32p, C.c_float, f32p]),
        }
        for k, (res, args) in sig.items():
            f = getattr(L, k)
            f.restype = res
            f.argtypes = args
        _g = L
    return _g


def _cam12(fov, eye, spot, up, near=0.0, far=float(np.finfo(np.float32).max)):
    return np.array([fov, *eye, *spot, *up, near, far], np.float32)


def _f(a, shape=None):
    a = np.ascontiguousarray(np.asarray(a, np.float32))
    return a if shape is None else np.ascontiguousarray(a.reshape(shape))


def ref_gen_rays(cam, film_w, film_h, nx, ny, four=True):
    """Camera{fov, eye, spot, up[, near, far]}.gen_rays4 / gen_rays1 of the
    reference on every pixel -> (ny, nx, k, 8)."""
    k = 4 if four else 1
    out = np.zeros((ny, nx, k, 8), np.float32)
    c = _cam12(*cam)
    reference_gi().rgi_gen_rays(_p(c, f32p), int(four), film_w, film_h, nx, ny, _p(out, f32p))
    return out


def ref_make_ray(o, d, tmin, tmax):
    out = np.zeros(8, np.float32)
    reference_gi().rgi_make_ray(_p(_f(o), f32p), _p(_f(d), f32p), tmin, tmax, _p(out, f32p))
    return out


def ref_aabb_isect(boxes, rays):
    """AABB3D::isect(ray, nullptr) for n (box, ray) pairs -> (n,) 0/1."""
    boxes, rays = _f(boxes, (-1, 6)), _f(rays, (-1, 8))
    assert len(boxes) == len(rays)
    out = np.zeros(len(rays), np.int32)
    reference_gi().rgi_aabb_isect(_p(boxes, f32p), _p(rays, f32p), len(rays), _p(out, i32p))
    return out


def ref_travorder(boxes, rays):
    """gi::travorder on gi::split's children of each box -> (order (n, 8),
    child boxes (n, 8, 6))."""
    boxes, rays = _f(boxes, (-1, 6)), _f(rays, (-1, 8))
    assert len(boxes) == len(rays)
    ord_ = np.zeros((len(rays), 8), np.int32)
    child = np.zeros((len(rays), 8, 6), np.float32)
    reference_gi().rgi_travorder(_p(boxes, f32p), _p(rays, f32p), len(rays), _p(ord_, i32p), _p(child, f32p))
    return ord_, child


def ref_film_add(film_w, film_h, nx, ny, xy, color):
    """Film::add per (x, y) / colour in order, then to_float_array."""
    xy = np.ascontiguousarray(np.asarray(xy, np.int32).reshape(-1, 2))
    color = _f(color, (-1, 3))
    out = np.zeros((ny, nx, 3), np.float32)
    reference_gi().rgi_film_add(film_w, film_h, nx, ny, _p(xy, i32p), _p(color, f32p), len(xy), _p(out, f32p))
    return out


def ref_probe_isect(probe, rays, prev):
    rays, prev = _f(rays, (-1, 8)), _f(prev, (-1, 3))
    hit = np.zeros(len(rays), np.int32)
    out = np.zeros((len(rays), 6), np.float32)
    reference_gi().rgi_probe_isect(_p(_f(probe), f32p), _p(rays, f32p), _p(prev, f32p), len(rays), _p(hit, i32p),
                                   _p(out, f32p))
    return hit, out[:, :3].copy(), out[:, 3:].copy()


def ref_probe_overlap(probe, boxes):
    boxes = _f(boxes, (-1, 6))
    out = np.zeros(len(boxes), np.int32)
    reference_gi().rgi_probe_overlap(_p(_f(probe), f32p), _p(boxes, f32p), len(boxes), _p(out, i32p))
    return out


def ref_probe_eval(sgs, dirs):
    """LightProbe::eval with the 14 SGs (14, 7) {a, d, s} on (m, 3) dirs."""
    sgs, dirs = _f(sgs, (14, 7)), _f(dirs, (-1, 3))
    out = np.zeros((len(dirs), 3), np.float32)
    reference_gi().rgi_probe_eval(_p(sgs, f32p), _p(dirs, f32p), len(dirs), _p(out, f32p))
    return out


def ref_sg_ops(lhs, rhs, dirs):
    """(lhs.eval(dir), lhs.integral(), prod(lhs, rhs) as (n, 7), inner_prod)."""
    lhs, rhs, dirs = _f(lhs, (-1, 7)), _f(rhs, (-1, 7)), _f(dirs, (-1, 3))
    n = len(lhs)
    ev, it, ip = (np.zeros((n, 3), np.float32) for _ in range(3))
    pr = np.zeros((n, 7), np.float32)
    reference_gi().rgi_sg_ops(_p(lhs, f32p), _p(rhs, f32p), _p(dirs, f32p), n, _p(ev, f32p), _p(it, f32p),
                              _p(pr, f32p), _p(ip, f32p))
    return ev, it, pr, ip


class RefScene:
    """The reference's own gi::Triangle / gi::LightProbe list and VoxelOctree
    over the arrays Scene takes.  texnames: per material a file for the
    reference's texel_fetch, or None / "" for an untextured material."""

    def __init__(self, sd, max_depth, probes=None, texnames=None):
        L = reference_gi()
        self.max_depth = int(max_depth)
        self.ntri = sd.ntri
        uv = sd.uv if sd.uv is not None else np.zeros((sd.ntri, 6), np.float32)
        mat = sd.mat if sd.mat is not None else np.zeros(sd.ntri, np.int32)
        nmat = len(sd.mat_tex)
        if texnames is None:
            if np.any(np.asarray(sd.mat_tex) >= 0):
                raise ValueError("textured materials need texnames (files the reference loads)")
            texnames = [None] * nmat
        names = (C.c_char_p * max(nmat, 1))(*[(t or "").encode() for t in texnames])
        pr = None if probes is None else _f(probes, (-1, 4))
        self.nprobe = 0 if pr is None else len(pr)
        self.h = L.rgi_scene_create(_p(_f(sd.pos), f32p), _p(_f(sd.nrm), f32p), _p(_f(uv), f32p),
                                    _p(np.ascontiguousarray(mat, np.int32), i32p), sd.ntri, nmat,
                                    _p(_f(sd.mat_kd), f32p), names, _p(pr, f32p), self.nprobe, self.max_depth)

    def close(self):
        if self.h:
            reference_gi().rgi_scene_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def dump(self):
        """Every node, children 0..7 below their parent: key (depth << 32 |
        code), leaf flag, box (n, 6), coverage, illum (n, 6, 3), voxel-list
        lengths and the lists one after another."""
        info = np.zeros(2, np.int64)
        reference_gi().rgi_tree_info(self.h, _p(info, i64p))
        n, r = int(info[0]), int(info[1])
        d = {"key": np.zeros(n, np.uint64), "leaf": np.zeros(n, np.int32), "box": np.zeros((n, 6), np.float32),
             "cov": np.zeros(n, np.float32), "illum": np.zeros((n, 6, 3), np.float32),
             "cnt": np.zeros(n, np.int32), "vox": np.zeros(max(r, 1), np.int32)}
        reference_gi().rgi_tree_dump(self.h, d["key"].ctypes.data_as(C.POINTER(C.c_uint64)), _p(d["leaf"], i32p),
                                     _p(d["box"], f32p), _p(d["cov"], f32p), _p(d["illum"], f32p),
                                     _p(d["cnt"], i32p), _p(d["vox"], i32p))
        d["vox"] = d["vox"][:r]
        return d

    def leaves(self):
        """As Scene.leaves(): the non-empty leaves sorted by code -> (vox, cnt,
        lists in list order)."""
        d = self.dump()
        sel = np.flatnonzero((d["leaf"] == 1) & (d["cnt"] > 0))
        off = np.concatenate([[0], np.cumsum(d["cnt"])])
        code = (d["key"][sel] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        o = np.argsort(code, kind="stable")
        lists = [d["vox"][off[i]:off[i + 1]] for i in sel[o]]
        return code[o], d["cnt"][sel[o]].astype(np.uint32), (np.concatenate(lists) if lists else np.zeros(0, np.int32))

    def boxes(self):
        """As Scene.boxes(): (key, box) of every node, sorted by key."""
        d = self.dump()
        o = np.argsort(d["key"], kind="stable")
        return d["key"][o], d["box"][o]

    def lightmap_nodes(self):
        """As Scene.lightmap_nodes(): (key, coverage, illum) sorted by key."""
        d = self.dump()
        o = np.argsort(d["key"], kind="stable")
        return d["key"][o], d["cov"][o], d["illum"][o]

    def ray_march(self, rays, even_invisible=False, pieces=False, color=(1.0, 1.0, 1.0)):
        """gi::ray_march per ray -> hit, tri (voxel index; probe k: ntri + k),
        voxel (the leaf's code), hit_p, normal; pieces=True adds get_diffuse
        (with color), get_albedo, is_visible and the leaf's compute_illum(-d)."""
        rays = _f(rays, (-1, 8))
        n = len(rays)
        r = {"hit": np.zeros(n, np.int32), "tri": np.zeros(n, np.int32), "voxel": np.zeros(n, np.uint32),
             "hit_p": np.zeros((n, 3), np.float32), "normal": np.zeros((n, 3), np.float32)}
        if pieces:
            r.update(diffuse=np.zeros((n, 3), np.float32), albedo=np.zeros((n, 3), np.float32),
                     visible=np.zeros(n, np.int32), illum=np.zeros((n, 3), np.float32))
        col = _f(color)
        reference_gi().rgi_ray_march(self.h, _p(rays, f32p), n, int(bool(even_invisible)), _p(col, f32p),
                                     _p(r["hit"], i32p), _p(r["tri"], i32p), _p(r["voxel"], u32p),
                                     _p(r["hit_p"], f32p), _p(r["normal"], f32p), _p(r.get("diffuse"), f32p),
                                     _p(r.get("albedo"), f32p), _p(r.get("visible"), i32p), _p(r.get("illum"), f32p))
        return r

    def lightmap(self, cam, film_w, film_h, nx, ny, color=(1.0, 1.0, 1.0), filter=True):
        """The light block in the canonical serial order, adding to the tree's
        illum (+ cone_trace_init_filter); returns the hit count."""
        c, col = _cam12(*cam), _f(color)
        hits = reference_gi().rgi_lightmap(self.h, _p(c, f32p), film_w, film_h, nx, ny, _p(col, f32p))
        if filter:
            reference_gi().rgi_lightmap_filter(self.h)
        return int(hits)

    def filter(self):
        reference_gi().rgi_lightmap_filter(self.h)

    def min_voxel(self, levels=None):
        return float(reference_gi().rgi_min_voxel(self.h, self.max_depth if levels is None else int(levels)))

    def cone_trace(self, hit_p, normal, min_voxel):
        q = np.ascontiguousarray(np.concatenate([_f(hit_p, (-1, 3)), _f(normal, (-1, 3))], axis=1))
        out = np.zeros((len(q), 3), np.float32)
        reference_gi().rgi_cone_trace(self.h, _p(q, f32p), len(q), min_voxel, _p(out, f32p))
        return out

    def probe_gather(self, probes, res, light_color, light_dir=(0.0, 1.0, 0.0)):
        """LightProbe{o, r}.gather_light per probe -> dict a, d (n, 14, 3), s (n, 14)."""
        pr = _f(probes, (-1, 4))
        sgs = np.zeros((len(pr), 14, 7), np.float32)
        reference_gi().rgi_probe_gather(self.h, _p(pr, f32p), len(pr), res, _p(_f(light_dir), f32p),
                                        _p(_f(light_color), f32p), _p(sgs, f32p))
        return {"a": sgs[:, :, 0:3].copy(), "d": sgs[:, :, 3:6].copy(), "s": sgs[:, :, 6].copy()}

    def gather_probes(self, res, light_color, light_dir=(0.0, 1.0, 0.0)):
        """gather_light for the scene's own probes, kept in them."""
        sgs = np.zeros((self.nprobe, 14, 7), np.float32)
        for k in range(self.nprobe):
            reference_gi().rgi_scene_probe_gather(self.h, k, res, _p(_f(light_dir), f32p), _p(_f(light_color), f32p),
                                                  _p(sgs[k], f32p))
        return {"a": sgs[:, :, 0:3].copy(), "d": sgs[:, :, 3:6].copy(), "s": sgs[:, :, 6].copy()}


class _RefObj(C.Structure):
    _fields_ = [("ok", C.c_int32), ("nv", C.c_int64), ("nvn", C.c_int64), ("nvt", C.c_int64),
                ("v", f32p), ("vn", f32p), ("vt", f32p), ("nshape", C.c_int32), ("nface", C.c_int64),
                ("fv", i32p), ("idx", i32p), ("mat", i32p), ("shape", i32p), ("nmat", C.c_int32),
                ("kd", f32p), ("name", C.POINTER(C.c_char_p)), ("tex", C.POINTER(C.c_char_p)),
                ("warn", C.c_char_p), ("err", C.c_char_p)]


def ref_load_obj(path, mtl_basedir):
    """tinyobj::LoadObj(.., path, mtl_basedir, triangulate=true) of the
    reference (compiled in place), flattened to numpy."""
    L = reference()
    q = L.ref_load_obj(str(path).encode(), None if mtl_basedir is None else str(mtl_basedir).encode())
    o = q.contents
    try:
        def arr(p, n, dt):
            return np.ctypeslib.as_array(p, (n,)).astype(dt) if n else np.zeros(0, dt)
        out = {"ok": bool(o.ok), "v": arr(o.v, o.nv * 3, np.float32).reshape(-1, 3),
               "vn": arr(o.vn, o.nvn * 3, np.float32).reshape(-1, 3),
               "vt": arr(o.vt, o.nvt * 2, np.float32).reshape(-1, 2), "nshape": o.nshape,
               "fv": arr(o.fv, o.nface, np.int32), "idx": arr(o.idx, o.nface * 9, np.int32).reshape(-1, 3, 3),
               "mat": arr(o.mat, o.nface, np.int32), "shape": arr(o.shape, o.nface, np.int32),
               "kd": arr(o.kd, o.nmat * 3, np.float32).reshape(-1, 3),
               "names": [o.name[i].decode(errors="surrogateescape") for i in range(o.nmat)],
               "texnames": [o.tex[i].decode(errors="surrogateescape") for i in range(o.nmat)],
               "warn": o.warn.decode(errors="replace"), "err": o.err.decode(errors="replace")}
    finally:
        L.ref_free_obj(q)
    return out


def _stbi_out(L, p, w, h, c):
    if not p:
        return None, L.ref_stbi_failure().decode()
    try:
        a = np.ctypeslib.as_array(p, (w.value * h.value * c.value,)).copy()
    finally:
        L.ref_stbi_free(p)
    return a.reshape(h.value, w.value, c.value), ""


def ref_stbi_load(path):
    """stbi_load(path, &w, &h, &c, 0) -> (uint8 (h, w, c) or None, failure reason)."""
    L = reference()
    w, h, c = C.c_int(), C.c_int(), C.c_int()
    p = L.ref_stbi_load(str(path).encode(), C.byref(w), C.byref(h), C.byref(c))
    return _stbi_out(L, p, w, h, c)


def ref_stbi_load_mem(data):
    L = reference()
    buf = np.frombuffer(bytes(data), np.uint8).copy()
    w, h, c = C.c_int(), C.c_int(), C.c_int()
    p = L.ref_stbi_load_mem(_p(buf, u8p) if buf.size else (C.c_uint8 * 1)(), buf.size, C.byref(w), C.byref(h),
                            C.byref(c))
    return _stbi_out(L, p, w, h, c)


# ---------------------------------------------------------------- primitives
def intersect_triangle3(q):
    """q: (15,) float64 {orig, dir, v0, v1, v2} -> (ret, t, u, v)."""
    q = np.ascontiguousarray(q, np.float64)
    t, u, v = C.c_double(), C.c_double(), C.c_double()
    r = oracle().ora_intersect_triangle3(*[_p(q[3 * k:3 * k + 3], f64p) for k in range(5)],
                                         C.byref(t), C.byref(u), C.byref(v))
    return r, t.value, u.value, v.value


def tri_box_overlap(q):
    """q: (15,) float32 {center, half, tri[9]} -> 1/0."""
    q = np.ascontiguousarray(q, np.float32)
    return oracle().ora_tri_box_overlap(_p(q[0:3], f32p), _p(q[3:6], f32p), _p(q[6:15], f32p))


def ref_intersect_triangle3(q):
    q = np.ascontiguousarray(q, np.float64)
    out = np.zeros(3)
    r = reference().ref_intersect_triangle3(*[_p(q[3 * k:3 * k + 3], f64p) for k in range(5)],
                                            _p(out, f64p), None)
    return r, out[0], out[1], out[2]


def ref_tri_box_overlap(q):
    q = np.ascontiguousarray(q, np.float32)
    return reference().ref_tri_box_overlap(_p(q[0:3], f32p), _p(q[3:6], f32p), _p(q[6:15], f32p))


def ref_hdr_bytes(img):
    img = np.ascontiguousarray(np.asarray(img, np.float32))
    h, w = img.shape[:2]
    comp = 1 if img.ndim == 2 else img.shape[2]
    n = reference().ref_write_hdr_mem(w, h, comp, _p(img, f32p), None, 0)
    buf = np.zeros(-n, np.uint8)
    n2 = reference().ref_write_hdr_mem(w, h, comp, _p(img, f32p), _p(buf, u8p), -n)
    assert n2 == -n
    return buf.tobytes()


def linear_to_rgbe_img(img):
    """stbiw__linear_to_rgbe per pixel of an (h, w, comp) float image ->
    (h, w, 4) uint8 (comp 1/2: grey; comp >= 3: first three channels)."""
    img = np.asarray(img, np.float32)
    if img.ndim == 2:
        img = img[:, :, None]
    h, w, c = img.shape
    lin = np.ascontiguousarray(np.repeat(img[:, :, :1], 3, 2) if c < 3 else img[:, :, :3]).reshape(-1, 3)
    out = np.zeros((h * w, 4), np.uint8)
    f = oracle().ora_linear_to_rgbe
    for i in range(h * w):
        f(_p(lin[i], f32p), _p(out[i], u8p))
    return out.reshape(h, w, 4)


def uniform_draws(seed, n):
    st = C.c_uint64(seed)
    return np.array([oracle().ora_uniform_m11(C.byref(st)) for _ in range(n)], np.float32)


def sphere_points(seed, n):
    st = C.c_uint64(seed)
    out = np.zeros((n, 3), np.float32)
    for i in range(n):
        oracle().ora_random_point_in_unit_sphere(C.byref(st), _p(out[i], f32p))
    return out


# ---------------------------------------------------------------- camera
def camera(fov, eye, spot, up, near=0.0, far=float(np.finfo(np.float32).max)):
    cam = np.zeros(19, np.float32)
    e, s, u = (np.ascontiguousarray(np.asarray(x, np.float32)) for x in (eye, spot, up))
    oracle().ora_camera_init(float(fov), _p(e, f32p), _p(s, f32p), _p(u, f32p), float(near), float(far),
                             _p(cam, f32p))
    return cam


def gen_rays4(cam, film_w, film_h, nx, ny, px, py):
    out = np.zeros((4, 8), np.float32)
    oracle().ora_gen_rays4(_p(cam, f32p), film_w, film_h, nx, ny, px, py, _p(out, f32p))
    return out


def gen_rays1(cam, film_w, film_h, nx, ny, px, py):
    out = np.zeros((1, 8), np.float32)
    oracle().ora_gen_rays1(_p(cam, f32p), film_w, film_h, nx, ny, px, py, _p(out, f32p))
    return out


def make_ray(o, d, tmin, tmax):
    out = np.zeros(8, np.float32)
    o = np.ascontiguousarray(o, np.float32)
    d = np.ascontiguousarray(d, np.float32)
    oracle().ora_make_ray(_p(o, f32p), _p(d, f32p), tmin, tmax, _p(out, f32p))
    return out


def aabb_isect(box, ray):
    box = np.ascontiguousarray(box, np.float32)
    ray = np.ascontiguousarray(ray, np.float32)
    return oracle().ora_aabb_isect(_p(box, f32p), _p(ray, f32p))


# ---------------------------------------------------------------- scene
class Scene:
    """The oracle's octree over a SceneData-like object."""

    def __init__(self, sd, max_depth):
        L = oracle()
        self.sd = sd
        self.max_depth = int(max_depth)
        uv = sd.uv if sd.uv is not None else np.zeros((sd.ntri, 6), np.float32)
        mat = sd.mat if sd.mat is not None else np.zeros(sd.ntri, np.int32)
        self._uv, self._mat = np.ascontiguousarray(uv), np.ascontiguousarray(mat)
        self.h = L.ora_scene_create(_p(sd.pos, f32p), _p(sd.nrm, f32p), _p(self._uv, f32p),
                                    _p(self._mat, i32p), sd.ntri, max_depth)
        ntex = len(sd.tex_off)
        L.ora_scene_set_materials(self.h, len(sd.mat_tex), _p(sd.mat_tex, i32p), _p(sd.mat_kd, f32p), ntex,
                                  _p(sd.tex_dims, i32p) if ntex else None,
                                  _p(sd.tex_off, i64p) if ntex else None,
                                  _p(sd.tex_data, u8p) if ntex else None, int(sd.tex_data.size))

    def close(self):
        if self.h:
            oracle().ora_scene_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        info = np.zeros(5, np.int64)
        box = np.zeros(6, np.float32)
        oracle().ora_scene_info(self.h, _p(info, i64p), _p(box, f32p))
        return info, box

    def leaves(self):
        info, _ = self.info()
        vox = np.zeros(info[3], np.uint32)
        cnt = np.zeros(info[3], np.uint32)
        tris = np.zeros(max(info[4], 1), np.int32)
        oracle().ora_scene_leaves(self.h, _p(vox, u32p), _p(cnt, u32p), _p(tris, i32p))
        return vox, cnt, tris[:info[4]]

    def boxes(self):
        """(key depth<<32|vox, box (n, 6)) of every node, sorted by key."""
        n = int(self.info()[0][0])
        key = np.zeros(n, np.uint64)
        box = np.zeros((n, 6), np.float32)
        oracle().ora_scene_boxes(self.h, key.ctypes.data_as(C.POINTER(C.c_uint64)), _p(box, f32p))
        o = np.argsort(key, kind="stable")
        return key[o], box[o]

    def ray_march(self, rays):
        rays = np.ascontiguousarray(np.asarray(rays, np.float32).reshape(-1, 8))
        n = rays.shape[0]
        hit = np.zeros(n, np.int32)
        tri = np.zeros(n, np.int32)
        vox = np.zeros(n, np.uint32)
        hp = np.zeros((n, 3), np.float32)
        nr = np.zeros((n, 3), np.float32)
        cnt = np.zeros((n, 4), np.uint32)
        oracle().ora_ray_march(self.h, _p(rays, f32p), n, _p(hit, i32p), _p(tri, i32p), _p(vox, u32p),
                               _p(hp, f32p), _p(nr, f32p), _p(cnt, u32p))
        return {"hit": hit, "tri": tri, "voxel": vox, "hit_p": hp, "normal": nr, "counters": cnt}

    def shade(self, rays):
        rays = np.ascontiguousarray(np.asarray(rays, np.float32).reshape(-1, 8))
        out = np.zeros((rays.shape[0], 3), np.float32)
        oracle().ora_shade(self.h, _p(rays, f32p), rays.shape[0], _p(out, f32p))
        return out

    def render(self, cam, film_w, film_h, nx, ny, film_index=1, nthreads=8, samples=True):
        rgb = np.zeros((ny, nx, 3), np.float32)
        ns = nx * ny * 4
        so = None
        if samples:
            so = {"hit": np.zeros(ns, np.int32), "tri": np.zeros(ns, np.int32),
                  "voxel": np.zeros(ns, np.uint32), "rgb": np.zeros((ns, 3), np.float32),
                  "counters": np.zeros((ns, 4), np.uint32)}
        oracle().ora_render(self.h, _p(cam, f32p), film_w, film_h, nx, ny, film_index, nthreads,
                            _p(rgb, f32p),
                            _p(so["hit"], i32p) if so else None, _p(so["tri"], i32p) if so else None,
                            _p(so["voxel"], u32p) if so else None, _p(so["rgb"], f32p) if so else None,
                            _p(so["counters"], u32p) if so else None)
        return (rgb, so) if so else rgb

    def render_secondary(self, cam, film_w, film_h, nx, ny, spp=64, nthreads=8, ids=True):
        vis = np.zeros((ny, nx), np.float32)
        ns = nx * ny * spp
        d = {"hit": np.zeros(ns, np.int32), "tri": np.zeros(ns, np.int32),
             "voxel": np.zeros(ns, np.uint32)} if ids else None
        rays = oracle().ora_render_secondary(self.h, _p(cam, f32p), film_w, film_h, nx, ny, spp, nthreads,
                                             _p(vis, f32p), _p(d["hit"], i32p) if d else None,
                                             _p(d["tri"], i32p) if d else None,
                                             _p(d["voxel"], u32p) if d else None)
        return (vis, rays, d) if ids else (vis, rays)

    def render_rows(self, cam, film_w, film_h, nx, ny, row_stride, row_phase, nthreads):
        rgb = np.zeros((ny, nx, 3), np.float32)
        sec = oracle().ora_render_rows(self.h, _p(cam, f32p), film_w, film_h, nx, ny, row_stride,
                                       row_phase, nthreads, _p(rgb, f32p))
        return sec, rgb

    # ---- full trace() ----
    def lightmap(self, cam, film_w, film_h, nx, ny, nthreads=8, filter=True):
        """Light pass in canonical order (+ cone_trace_init_filter); returns hits."""
        hits = oracle().ora_lightmap(self.h, _p(cam, f32p), film_w, film_h, nx, ny, nthreads)
        if filter:
            oracle().ora_lightmap_filter(self.h)
        return hits

    def lightmap_nodes(self):
        """(key depth<<32|vox, coverage, illum (n,6,3)) sorted by key."""
        n = int(self.info()[0][0])
        key = np.zeros(n, np.uint64)
        cov = np.zeros(n, np.float32)
        ill = np.zeros((n, 6, 3), np.float32)
        oracle().ora_lightmap_nodes(self.h, key.ctypes.data_as(C.POINTER(C.c_uint64)), _p(cov, f32p),
                                    _p(ill, f32p))
        o = np.argsort(key, kind="stable")
        return key[o], cov[o], ill[o]

    def min_voxel(self, levels=None):
        return float(oracle().ora_min_voxel(self.h, self.max_depth if levels is None else int(levels)))

    def cone_trace(self, hit_p, normal, min_voxel):
        """gi::cone_trace(root, isect, min_voxel) at (n, 3) points / normals."""
        q = np.ascontiguousarray(np.concatenate([np.asarray(hit_p, np.float32).reshape(-1, 3),
                                                 np.asarray(normal, np.float32).reshape(-1, 3)], axis=1))
        out = np.zeros((len(q), 3), np.float32)
        oracle().ora_cone_trace(self.h, _p(q, f32p), len(q), min_voxel, _p(out, f32p))
        return out

    def hit_pieces(self, rays):
        """Per ray (+0 on a miss): get_diffuse under white, get_albedo and the
        hit leaf's compute_illum(-d)."""
        rays = np.ascontiguousarray(np.asarray(rays, np.float32).reshape(-1, 8))
        d, a, i = (np.zeros((len(rays), 3), np.float32) for _ in range(3))
        oracle().ora_hit_pieces(self.h, _p(rays, f32p), len(rays), _p(d, f32p), _p(a, f32p), _p(i, f32p))
        return {"diffuse": d, "albedo": a, "illum": i}

    def shade_trace(self, rays, res):
        rays = np.ascontiguousarray(np.asarray(rays, np.float32).reshape(-1, 8))
        out = np.zeros((rays.shape[0], 3), np.float32)
        oracle().ora_shade_trace(self.h, _p(rays, f32p), rays.shape[0], res, _p(out, f32p))
        return out

    def render_trace(self, cam, film_w, film_h, nx, ny, res, nthreads=8, samples=True):
        rgb = np.zeros((ny, nx, 3), np.float32)
        ns = nx * ny * 4
        hit = np.zeros(ns, np.int32) if samples else None
        srgb = np.zeros((ns, 3), np.float32) if samples else None
        oracle().ora_render_trace(self.h, _p(cam, f32p), film_w, film_h, nx, ny, res, nthreads, _p(rgb, f32p),
                                  _p(hit, i32p), _p(srgb, f32p))
        return (rgb, {"hit": hit, "rgb": srgb}) if samples else rgb
