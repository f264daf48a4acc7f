"""Python mirror of the reference's hot-path interface over libvrt.so.

Names follow the reference (VRT/x = VoxelRayTrace20190722/x):
  Camera(fov, eye, spot, up, near, far), Camera.gen_rays4/gen_rays1  VRT/camera.h:70-84
  Film(w, h, nx, ny)                                                 VRT/camera.h:24-39
  ray_march_init(scene, max_depth) -> VoxelOctree                    VRT/voxel_octree.h:85-86
  ray_march(tree, rays)                                              VRT/voxel_octree.h:87-89
  trace(tree, rays) / cone_trace(tree, hit_p, normal)                VRT/main.cc:10-30, voxel_octree.cc:313-330
  render(tree, cam, film)     the per-pixel loop of VRT/main.cc:118-123 (primary shading)
  intersect_triangle3 / tri_box_overlap                              VRT/raytri.h:5, tribox2.h:6
  write_hdr                                                          VRT/stb_image_write.h:178
Errors raise VrtError (the reference exit()s or returns false).
"""
import ctypes as C
import numpy as np

from . import _ffi
from ._ffi import VrtError, check, lib, ptr

FLT_MAX = float(np.finfo(np.float32).max)
# the usual one-lobe fit of a clamped cosine (VoxelOctree.probe_irradiance's default lobe)
SG_COSINE_AMPLITUDE = 1.17   # include/vrt.h VRT_SG_COSINE_AMPLITUDE
SG_COSINE_SHARPNESS = 2.133  # include/vrt.h VRT_SG_COSINE_SHARPNESS


def to_radian(degree):
    """jql::to_radian: degree * pi / 180.f in float (VRT/graphics_math.h:896-899)."""
    d = np.float32(degree)
    return float(np.float32(np.float32(d * np.float32(3.1415926535897932384626)) / np.float32(180.0)))


def _f3(v):
    a = np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(3))
    return a


class Film:
    """Film(w, h, nx, ny) (VRT/camera.h:24-39)."""

    def __init__(self, w, h, nx, ny):
        self.w, self.h, self.nx, self.ny = float(w), float(h), int(nx), int(ny)
        self.c = _ffi.Film(self.w, self.h, self.nx, self.ny)


class Camera:
    """Camera(fov, eye, spot, up, near=0, far=FLT_MAX) (VRT/camera.cc:65-75)."""

    def __init__(self, fov, eye, spot, up, near=0.0, far=FLT_MAX):
        self.c = _ffi.Camera()
        self.eye, self.spot, self.up = _f3(eye), _f3(spot), _f3(up)
        check(lib().vrt_camera_init(float(fov), ptr(self.eye, _ffi.f32p), ptr(self.spot, _ffi.f32p),
                                    ptr(self.up, _ffi.f32p), float(near), float(far),
                                    C.byref(self.c)), "vrt_camera_init")

    @staticmethod
    def _rays(arr):
        out = np.zeros((len(arr), 8), dtype=np.float32)
        for i, r in enumerate(arr):
            out[i, 0:3] = r.o[:]
            out[i, 3:6] = r.d[:]
            out[i, 6] = r.tmin
            out[i, 7] = r.tmax
        return out

    def gen_rays4(self, film, px, py):
        """4 rays {o, d, tmin, tmax} as a (4, 8) float32 array (VRT/camera.cc:95-112)."""
        arr = (_ffi.Ray * 4)()
        check(lib().vrt_gen_rays4(C.byref(self.c), C.byref(film.c), int(px), int(py), arr),
              "vrt_gen_rays4")
        return self._rays(arr)

    def defer_bound(self, film):
        """vrt_camera_defer_bound: an upper bound on the rays of the film the
        fast-only render defers (0: no deferred pass is launched)."""
        n = C.c_int64()
        check(lib().vrt_camera_defer_bound(C.byref(self.c), C.byref(film.c), C.byref(n)), "vrt_camera_defer_bound")
        return n.value

    def gen_rays1(self, film, px, py):
        arr = (_ffi.Ray * 1)()
        check(lib().vrt_gen_rays1(C.byref(self.c), C.byref(film.c), int(px), int(py), arr),
              "vrt_gen_rays1")
        return self._rays(arr)


class Light:
    """One light of a light list (vrt_light): a light camera, its film and the
    colour the light pass hands to Triangle::get_diffuse (the reference's
    driver passes (1, 1, 1)).  The colour is taken as it is."""

    def __init__(self, camera, film, color=(1.0, 1.0, 1.0)):
        self.camera, self.film, self.color = camera, film, _f3(color)


def _lights_arg(lights):
    """(vrt_light array or None, count) of a sequence of Light."""
    if lights is None:
        return None, 0
    lights = list(lights)
    arr = (_ffi.LightRec * max(1, len(lights)))()
    for i, l in enumerate(lights):
        arr[i].cam = l.camera.c
        arr[i].film = l.film.c
        arr[i].color[:] = [float(v) for v in l.color]
    return arr, len(lights)


def make_ray(o, d, tmin=0.0, tmax=FLT_MAX):
    """jql::Ray(o, d, tmin, tmax): normalises d (VRT/graphics_math.h:1159-1166)."""
    r = _ffi.Ray()
    o, d = _f3(o), _f3(d)
    check(lib().vrt_make_ray(ptr(o, _ffi.f32p), ptr(d, _ffi.f32p), float(tmin), float(tmax),
                             C.byref(r)), "vrt_make_ray")
    return np.array(list(r.o) + list(r.d) + [r.tmin, r.tmax], dtype=np.float32)


class SceneData:
    """Triangle soup + materials + textures (the obj2voxel output the
    reference builds its octree from, VRT/voxel_octree.cc:305-371)."""

    def __init__(self, pos, nrm, uv=None, mat=None, mat_tex=None, mat_kd=None,
                 tex_dims=None, tex_off=None, tex_data=None):
        self.pos = np.ascontiguousarray(np.asarray(pos, np.float32).reshape(-1, 9))
        n = self.pos.shape[0]
        self.nrm = np.ascontiguousarray(np.asarray(nrm, np.float32).reshape(n, 9))
        self.uv = None if uv is None else np.ascontiguousarray(np.asarray(uv, np.float32).reshape(n, 6))
        self.mat = None if mat is None else np.ascontiguousarray(np.asarray(mat, np.int32).reshape(n))
        self.mat_tex = np.ascontiguousarray(np.asarray([-1] if mat_tex is None else mat_tex, np.int32))
        self.mat_kd = np.ascontiguousarray(
            np.asarray([[0.8, 0.8, 0.8]] if mat_kd is None else mat_kd, np.float32).reshape(-1, 3))
        self.tex_dims = np.ascontiguousarray(np.asarray([] if tex_dims is None else tex_dims,
                                                        np.int32).reshape(-1, 3))
        self.tex_off = np.ascontiguousarray(np.asarray([] if tex_off is None else tex_off, np.int64))
        self.tex_data = np.ascontiguousarray(np.asarray([] if tex_data is None else tex_data, np.uint8))

    @property
    def ntri(self):
        return self.pos.shape[0]

    def desc(self):
        d = _ffi.SceneDesc()
        d.ntri = self.ntri
        d.pos = ptr(self.pos, _ffi.f32p)
        d.nrm = ptr(self.nrm, _ffi.f32p)
        d.uv = ptr(self.uv, _ffi.f32p)
        d.mat = ptr(self.mat, _ffi.i32p)
        d.nmat = len(self.mat_tex)
        d.mat_tex = ptr(self.mat_tex, _ffi.i32p)
        d.mat_kd = ptr(self.mat_kd, _ffi.f32p)
        d.ntex = len(self.tex_off)
        d.tex_dims = ptr(self.tex_dims, _ffi.i32p) if len(self.tex_off) else None
        d.tex_off = ptr(self.tex_off, _ffi.i64p) if len(self.tex_off) else None
        d.tex_data = ptr(self.tex_data, _ffi.u8p) if len(self.tex_off) else None
        d.tex_bytes = int(self.tex_data.size)
        return d

    @classmethod
    def proxy(cls, detail=1.0, seed=1):
        """The deterministic sponza-proxy atrium (vrt_proxy_scene)."""
        L = lib()
        nt, nm, nx, tb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        check(L.vrt_proxy_scene(float(detail), int(seed), C.byref(nt), None, None, None, None,
                                C.byref(nm), None, None, C.byref(nx), None, None, None,
                                C.byref(tb)), "vrt_proxy_scene(count)")
        n = nt.value
        pos = np.zeros((n, 9), np.float32)
        nrm = np.zeros((n, 9), np.float32)
        uv = np.zeros((n, 6), np.float32)
        mat = np.zeros(n, np.int32)
        mt = np.zeros(nm.value, np.int32)
        kd = np.zeros((nm.value, 3), np.float32)
        td = np.zeros((nx.value, 3), np.int32)
        to = np.zeros(nx.value, np.int64)
        tx = np.zeros(tb.value, np.uint8)
        check(L.vrt_proxy_scene(float(detail), int(seed), C.byref(nt), ptr(pos, _ffi.f32p),
                                ptr(nrm, _ffi.f32p), ptr(uv, _ffi.f32p), ptr(mat, _ffi.i32p),
                                C.byref(nm), ptr(mt, _ffi.i32p), ptr(kd, _ffi.f32p), C.byref(nx),
                                ptr(td, _ffi.i32p), ptr(to, _ffi.i64p), ptr(tx, _ffi.u8p),
                                C.byref(tb)), "vrt_proxy_scene")
        return cls(pos, nrm, uv, mat, mt, kd, td, to, tx)

    @classmethod
    def from_obj(cls, path):
        """obj2voxel(path) + textures (VRT/voxel_octree.cc:305-388)."""
        with ObjModel(path) as m:
            return m.scene_data()


class ObjModel:
    """tinyobj::LoadObj result (+ the obj2voxel soup unless parse_only)
    through vrt_obj_load.  Usable as a context manager; arrays returned are
    copies, so they outlive the handle."""

    def __init__(self, path, parse_only=False):
        self.h = C.c_void_p()
        flags = _ffi.VRT_OBJ_PARSE_ONLY if parse_only else 0
        check(lib().vrt_obj_load(str(path).encode(), flags, C.byref(self.h)), f"vrt_obj_load({path})")
        self.info = _ffi.ObjInfo()
        check(lib().vrt_obj_info(self.h, C.byref(self.info)), "vrt_obj_info")

    def close(self):
        if self.h:
            lib().vrt_obj_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: module globals already gone
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def attrib(self):
        """(vertices (n,3), normals (n,3), texcoords (n,2)) float32."""
        v, vn, vt = _ffi.f32p(), _ffi.f32p(), _ffi.f32p()
        check(lib().vrt_obj_attrib(self.h, C.byref(v), C.byref(vn), C.byref(vt)), "vrt_obj_attrib")
        i = self.info

        def arr(p, n, k):
            if n == 0:
                return np.zeros((0, k), np.float32)
            return np.ctypeslib.as_array(p, (n * k,)).reshape(n, k).copy()
        return arr(v, i.nvert, 3), arr(vn, i.nnormal, 3), arr(vt, i.ntexcoord, 2)

    def faces(self):
        """Per triangle: idx (n,3,3) {v,vn,vt} per corner, material id, shape."""
        n = self.info.nface
        idx = np.zeros((n, 3, 3), np.int32)
        mat = np.zeros(n, np.int32)
        shp = np.zeros(n, np.int32)
        check(lib().vrt_obj_faces(self.h, ptr(idx, _ffi.i32p), ptr(mat, _ffi.i32p), ptr(shp, _ffi.i32p)),
              "vrt_obj_faces")
        return idx, mat, shp

    def materials(self):
        out = []
        for i in range(self.info.nmat):
            name, tex = C.c_char_p(), C.c_char_p()
            kd = np.zeros(3, np.float32)
            check(lib().vrt_obj_material(self.h, i, C.byref(name), ptr(kd, _ffi.f32p), C.byref(tex)),
                  "vrt_obj_material")
            out.append({"name": name.value.decode(errors="surrogateescape"), "kd": kd,
                        "texname": tex.value.decode(errors="surrogateescape")})
        return out

    def texture_paths(self):
        out = []
        for i in range(self.info.ntex):
            p = C.c_char_p()
            check(lib().vrt_obj_texture_path(self.h, i, C.byref(p)), "vrt_obj_texture_path")
            out.append(p.value.decode(errors="surrogateescape"))
        return out

    def warnings(self):
        return lib().vrt_obj_warnings(self.h).decode(errors="replace")

    def scene_data(self):
        d = _ffi.SceneDesc()
        check(lib().vrt_obj_scene_desc(self.h, C.byref(d)), "vrt_obj_scene_desc")
        n, nm, nt = d.ntri, d.nmat, d.ntex

        def cp(p, count, dt):
            if count == 0:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array(p, (count,)).copy()
        return SceneData(cp(d.pos, n * 9, np.float32), cp(d.nrm, n * 9, np.float32), cp(d.uv, n * 6, np.float32),
                         cp(d.mat, n, np.int32), cp(d.mat_tex, nm, np.int32), cp(d.mat_kd, nm * 3, np.float32),
                         cp(d.tex_dims, nt * 3, np.int32), cp(d.tex_off, nt, np.int64),
                         cp(d.tex_data, d.tex_bytes, np.uint8))


def obj2voxel(path):
    """The reference's obj2voxel (VRT/voxel_octree.cc:305-371) as SceneData."""
    return SceneData.from_obj(path)


def _image_out(rc, where, w, h, c, p):
    check(rc, where)
    try:
        n = w.value * h.value * c.value
        a = np.ctypeslib.as_array(p, (n,)).copy()
    finally:
        lib().vrt_image_free(p)
    return a.reshape(h.value, w.value, c.value)


def load_image(path):
    """stbi_load(path, .., 0) for TGA (VRT/voxel_octree.cc:373-388):
    uint8 (h, w, channels), row 0 = top."""
    w, h, c, p = C.c_int32(), C.c_int32(), C.c_int32(), _ffi.u8p()
    rc = lib().vrt_tga_load(str(path).encode(), C.byref(w), C.byref(h), C.byref(c), C.byref(p))
    return _image_out(rc, f"vrt_tga_load({path})", w, h, c, p)


def tga_decode(data):
    """stbi_load_from_memory for TGA bytes."""
    buf = np.frombuffer(bytes(data), np.uint8)
    w, h, c, p = C.c_int32(), C.c_int32(), C.c_int32(), _ffi.u8p()
    rc = lib().vrt_tga_decode(ptr(buf, _ffi.u8p) if buf.size else (C.c_uint8 * 1)(), buf.size, C.byref(w),
                              C.byref(h), C.byref(c), C.byref(p))
    return _image_out(rc, "vrt_tga_decode", w, h, c, p)


class VoxelOctree:
    """The octree built by gi::ray_march_init and resident on one device
    (device < 0: host-only, for inspecting the build)."""

    def __init__(self, scene, max_depth, device=0, build_on_device=False, probes=None):
        """probes: (n, 4) light probes {o, r} (or LightProbe objects) pushed
        into the voxel list behind the triangles, as VRT/main.cc:56-64 does:
        voxel ntri + k is probe k (vrt_scene_create_probes).  build_on_device
        builds the whole tree on the GPU, the probes included."""
        self.scene = scene  # keeps the arrays alive for the descriptor
        h = C.c_void_p()
        d = scene.desc()
        flags = _ffi.VRT_BUILD_DEVICE if build_on_device else 0
        self.probes = _probes_arg(probes)
        if build_on_device and self.probes is not None:
            flags |= _ffi.VRT_BUILD_DEVICE_PROBES
        if self.probes is None:
            check(lib().vrt_scene_create_ex(C.byref(d), int(max_depth), int(device), flags, C.byref(h)),
                  "vrt_scene_create")
        else:
            check(lib().vrt_scene_create_probes(C.byref(d), self.probes.ctypes.data_as(C.POINTER(_ffi.Probe)),
                                                len(self.probes), int(max_depth), int(device), flags, C.byref(h)),
                  "vrt_scene_create_probes")
        self.h = h
        self.max_depth = int(max_depth)
        self.info = _ffi.SceneInfo()
        check(lib().vrt_scene_info(self.h, C.byref(self.info)), "vrt_scene_info")

    _probes = None
    _probes_moved = False

    @property
    def probes(self):
        """The scene's probes as (n, 4) {o, r}, or None.  After an
        update_probes_device that moved them they are fetched from the scene's
        device copy, once, when first asked for."""
        if self._probes_moved:
            self._probes = np.ascontiguousarray(self.device_array(7).view(np.float32).reshape(-1, 4))
            self._probes_moved = False
        return self._probes

    @probes.setter
    def probes(self, value):
        self._probes = value
        self._probes_moved = False

    def close(self):
        if self.h:
            lib().vrt_scene_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def root_box(self):
        return (np.array(self.info.root_min[:], np.float32), np.array(self.info.root_max[:], np.float32))

    @property
    def chain_spacing(self):
        """The chain order's scene constant (vrt_scene_chain_spacing): per axis
        the smallest child-centre spacing of the internal nodes, zeros = off."""
        w = np.zeros(3, np.float32)
        check(lib().vrt_scene_chain_spacing(self.h, ptr(w, _ffi.f32p)), "vrt_scene_chain_spacing")
        return w

    @property
    def ref_record_bytes(self):
        """Bytes per leaf record of the device format (vrt_scene_ref_format):
        48, or 64 for scenes with large leaves."""
        v = C.c_int32()
        check(lib().vrt_scene_ref_format(self.h, C.byref(v)), "vrt_scene_ref_format")
        return v.value

    def nodes(self):
        """The flattened octree as uploaded: (boxes (n,6) f32, word a, word b) per
        node in BFS child-block order."""
        n = self.info.nodes
        box = np.zeros((n, 6), np.float32)
        a = np.zeros(n, np.uint32)
        b = np.zeros(n, np.uint32)
        check(lib().vrt_scene_nodes(self.h, ptr(box, _ffi.f32p), ptr(a, _ffi.u32p), ptr(b, _ffi.u32p)),
              "vrt_scene_nodes")
        return box, a, b

    def update(self, pos, nrm=None):
        """Rebuild the scene in place from new vertex positions (ntri*9 floats)
        and, unless nrm is None, new vertex normals (vrt_scene_update).
        Afterwards the tree equals one freshly built from these arrays; a
        refused update raises and leaves the previous geometry in place."""
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1)
        n9 = 9 * self.scene.ntri
        if pos.size != n9:
            raise ValueError(f"pos has {pos.size} floats, the scene needs {n9}")
        if nrm is not None:
            nrm = np.ascontiguousarray(nrm, np.float32).reshape(-1)
            if nrm.size != n9:
                raise ValueError(f"nrm has {nrm.size} floats, the scene needs {n9}")
        check(lib().vrt_scene_update(self.h, ptr(pos, _ffi.f32p), ptr(nrm, _ffi.f32p)), "vrt_scene_update")
        check(lib().vrt_scene_info(self.h, C.byref(self.info)), "vrt_scene_info")

    def update_device(self, d_pos_ptr, d_nrm_ptr=None, stream_ptr=None):
        """update() from device arrays on the scene's device, read in the order
        of stream_ptr (vrt_scene_update_device); ready on return."""
        check(lib().vrt_scene_update_device(self.h, C.c_void_p(d_pos_ptr),
                                            C.c_void_p(d_nrm_ptr) if d_nrm_ptr else None,
                                            C.c_void_p(stream_ptr) if stream_ptr else None),
              "vrt_scene_update_device")
        check(lib().vrt_scene_info(self.h, C.byref(self.info)), "vrt_scene_info")

    def update_probes(self, pos, nrm=None, probes=None):
        """update() for a scene with light probes (vrt_scene_update_probes):
        new positions, unless nrm is None new normals, and unless probes is
        None new probe centres and radii ((nprobe, 4) {o, r} or LightProbe
        objects).  Afterwards the scene equals one freshly built from these
        arrays, except that the stored SGs stay."""
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1)
        n9 = 9 * self.scene.ntri
        if pos.size != n9:
            raise ValueError(f"pos has {pos.size} floats, the scene needs {n9}")
        if nrm is not None:
            nrm = np.ascontiguousarray(nrm, np.float32).reshape(-1)
            if nrm.size != n9:
                raise ValueError(f"nrm has {nrm.size} floats, the scene needs {n9}")
        pp = None
        if probes is not None:
            probes = _probes_arg(probes)
            have = 0 if self.probes is None else len(self.probes)
            if probes is None or len(probes) != have:
                raise ValueError(f"probes has {0 if probes is None else len(probes)} records, the scene has {have}")
            pp = probes.ctypes.data_as(C.POINTER(_ffi.Probe))
        check(lib().vrt_scene_update_probes(self.h, ptr(pos, _ffi.f32p), ptr(nrm, _ffi.f32p), pp),
              "vrt_scene_update_probes")
        if probes is not None:
            self.probes = probes
        check(lib().vrt_scene_info(self.h, C.byref(self.info)), "vrt_scene_info")

    def update_probes_device(self, d_pos_ptr, d_nrm_ptr=None, d_probes_ptr=None, stream_ptr=None):
        """update_probes() from device arrays on the scene's device, read in
        the order of stream_ptr (vrt_scene_update_probes_device); ready on
        return.  self.probes is fetched again from the scene's device copy
        when it is next asked for, not here."""
        check(lib().vrt_scene_update_probes_device(self.h, C.c_void_p(d_pos_ptr),
                                                   C.c_void_p(d_nrm_ptr) if d_nrm_ptr else None,
                                                   C.c_void_p(d_probes_ptr) if d_probes_ptr else None,
                                                   C.c_void_p(stream_ptr) if stream_ptr else None),
              "vrt_scene_update_probes_device")
        if d_probes_ptr:
            self._probes_moved = True
        check(lib().vrt_scene_info(self.h, C.byref(self.info)), "vrt_scene_info")

    def update_stats(self):
        """The last update's wall-clock split in ms (vrt_scene_update_stats)."""
        ms = np.zeros(4, np.float64)
        check(lib().vrt_scene_update_stats(self.h, ptr(ms, _ffi.f64p)), "vrt_scene_update_stats")
        return dict(total=ms[0], gpu=ms[1], copy_back=ms[2], host=ms[3])

    def update_scratch(self, release=False):
        """Bytes of device memory the scene keeps for its next update, counted
        by neither info.device_bytes nor scratch_bytes(); release=True frees
        them (vrt_scene_update_scratch)."""
        nb = C.c_int64()
        check(lib().vrt_scene_update_scratch(self.h, int(bool(release)), C.byref(nb)), "vrt_scene_update_scratch")
        return nb.value

    def device_array(self, kind):
        """One derived device array as bytes (vrt_scene_device_array): 0 leaf
        records, 1 per-record boxes, 2 march records, 3 TriPos, 4 TriAttr; on a
        scene with probes also 5 pnode, 6 pref, 7 the probes."""
        nb = C.c_int64()
        check(lib().vrt_scene_device_array(self.h, int(kind), None, 0, C.byref(nb)), "vrt_scene_device_array")
        out = np.zeros(nb.value, np.uint8)
        check(lib().vrt_scene_device_array(self.h, int(kind), out.ctypes.data_as(C.c_void_p), nb.value,
                                           C.byref(nb)), "vrt_scene_device_array")
        return out

    def digest(self):
        """The ten digest words of the arrays an update rewrites
        (vrt_scene_digest): items 0-7 are device_array's kinds (an absent
        array digests to 0), 8 the node records, 9 the nodes' voxel indices."""
        out = np.zeros(DIGEST_ITEMS, np.uint64)
        check(lib().vrt_scene_digest(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64))), "vrt_scene_digest")
        return out

    def leaves(self):
        """(voxel ids, counts, concatenated triangle lists) of the non-empty leaves."""
        nl, nr = self.info.nonempty_leaves, self.info.tri_refs
        vox = np.zeros(nl, np.uint32)
        cnt = np.zeros(nl, np.uint32)
        tris = np.zeros(max(nr, 1), np.int32)
        check(lib().vrt_scene_leaves(self.h, ptr(vox, _ffi.u32p), ptr(cnt, _ffi.u32p),
                                     ptr(tris, _ffi.i32p)), "vrt_scene_leaves")
        return vox, cnt, tris[:nr]

    def probe_info(self):
        """(probes, leaves holding a probe, total length of their probe lists)."""
        n, nl, nr = C.c_int32(), C.c_int64(), C.c_int64()
        check(lib().vrt_scene_probe_info(self.h, C.byref(n), C.byref(nl), C.byref(nr)), "vrt_scene_probe_info")
        return n.value, nl.value, nr.value

    def probe_leaves(self):
        """(voxel ids, counts, concatenated probe lists) of the leaves that hold
        at least one probe, as leaves() is for the triangles."""
        _, nl, nr = self.probe_info()
        vox = np.zeros(max(nl, 1), np.uint32)
        cnt = np.zeros(max(nl, 1), np.uint32)
        pr = np.zeros(max(nr, 1), np.int32)
        check(lib().vrt_scene_probe_leaves(self.h, ptr(vox, _ffi.u32p), ptr(cnt, _ffi.u32p), ptr(pr, _ffi.i32p)),
              "vrt_scene_probe_leaves")
        return vox[:nl], cnt[:nl], pr[:nr]

    @property
    def probe_sgs(self):
        """The scene's stored SGs (zero at creation) as probe_gather's dict:
        a, d (n, 14, 3) and s (n, 14); a probe hit's get_albedo reads them."""
        n = self.probe_info()[0]
        sgs = np.zeros((max(n, 1), PROBE_SGS, 7), np.float32)
        check(lib().vrt_scene_probe_sgs(self.h, sgs.ctypes.data_as(C.POINTER(_ffi.SGRec))), "vrt_scene_probe_sgs")
        sgs = sgs[:n]
        return {"a": sgs[:, :, 0:3].copy(), "d": sgs[:, :, 3:6].copy(), "s": sgs[:, :, 6].copy()}

    @probe_sgs.setter
    def probe_sgs(self, sgs):
        n = self.probe_info()[0]
        a, d, s = (np.asarray(sgs[k], np.float32) for k in ("a", "d", "s"))
        if a.shape != (n, PROBE_SGS, 3) or d.shape != a.shape or s.shape != (n, PROBE_SGS):
            raise ValueError(f"sgs must hold a, d ({n}, 14, 3) and s ({n}, 14), got {a.shape}, {d.shape}, {s.shape}")
        rec = np.ascontiguousarray(np.concatenate([a, d, s[:, :, None]], axis=2))
        check(lib().vrt_scene_set_probe_sgs(self.h, rec.ctypes.data_as(C.POINTER(_ffi.SGRec))),
              "vrt_scene_set_probe_sgs")

    def gather_probes(self, res=0.0, light_color=(1.0, 1.0, 1.0)):
        """VRT/main.cc:104-105: gather_light for every probe of the scene (the
        reference's 100 points) into the stored SGs; returns them."""
        lc = _f3(light_color)
        check(lib().vrt_scene_probes_gather(self.h, float(res), ptr(lc, _ffi.f32p)), "vrt_scene_probes_gather")
        return self.probe_sgs

    def probe_shade_hits(self, hits, rgb, albedo=None):
        """vrt_probe_shade_hits: finish a trace_device batch on the host.  hits:
        the (n, 9) uint32 vrt_hit records copied back; rgb / albedo (n, 3)
        float32 arrays updated in place where a ray ended on a probe."""
        hits = np.ascontiguousarray(hits, np.uint32)
        for a in (rgb, albedo):
            if a is not None and not (a.dtype == np.float32 and a.flags.c_contiguous and a.shape == (len(hits), 3)):
                raise ValueError("rgb / albedo must be C-contiguous float32 (n, 3)")
        check(lib().vrt_probe_shade_hits(self.h, C.c_void_p(hits.ctypes.data), len(hits), ptr(rgb, _ffi.f32p),
                                         ptr(albedo, _ffi.f32p)), "vrt_probe_shade_hits")

    def probe_shade_hits_device(self, d_hits_ptr, n, d_rgb_ptr=None, d_albedo_ptr=None, stream_ptr=None):
        """vrt_probe_shade_hits_device: finish a trace_device batch where it
        lies (device pointers; d_rgb_ptr / d_albedo_ptr may be None)."""
        vp = lambda q: None if q is None else C.c_void_p(q)
        check(lib().vrt_probe_shade_hits_device(self.h, C.c_void_p(d_hits_ptr), int(n), vp(d_rgb_ptr),
                                                vp(d_albedo_ptr), vp(stream_ptr)), "vrt_probe_shade_hits_device")

    def probe_irradiance(self, hit_p, normal, lobe_a=(SG_COSINE_AMPLITUDE,) * 3, lobe_s=SG_COSINE_SHARPNESS,
                         counts=False):
        """vrt_probe_irradiance: the light the scene's probes send to (n, 3)
        points with (n, 3) normals -> (n, 3): the mean over the probes of the
        point's leaf of the sum over their stored lobes of inner_prod(lobe,
        SG{lobe_a, normal, lobe_s}); +0 where the leaf holds no probe.
        counts=True also returns the (n,) int32 probe counts."""
        hit_p, normal = np.asarray(hit_p, np.float32), np.asarray(normal, np.float32)
        if hit_p.ndim != 2 or hit_p.shape[1] != 3 or normal.shape != hit_p.shape:
            raise ValueError(f"hit_p and normal must both be (n, 3), got {hit_p.shape} and {normal.shape}")
        isects = np.ascontiguousarray(np.concatenate([hit_p, normal], axis=1))
        n = isects.shape[0]
        la = _f3(lobe_a)
        rgb = np.zeros((n, 3), np.float32)
        cnt = np.zeros(n, np.int32) if counts else None
        check(lib().vrt_probe_irradiance(self.h, isects.ctypes.data_as(C.POINTER(_ffi.ISect)), n, ptr(la, _ffi.f32p),
                                         float(lobe_s), ptr(rgb, _ffi.f32p), ptr(cnt, _ffi.i32p)),
              "vrt_probe_irradiance")
        return (rgb, cnt) if counts else rgb

    def probe_irradiance_device(self, d_isects_ptr, n, d_rgb_ptr, d_count_ptr=None,
                                lobe_a=(SG_COSINE_AMPLITUDE,) * 3, lobe_s=SG_COSINE_SHARPNESS, stream_ptr=None):
        """vrt_probe_irradiance_device: n vrt_isect {hit_p, normal} in, 3n
        floats and (unless d_count_ptr is None) n int32 counts out, device
        pointers, enqueued on the stream."""
        vp = lambda q: None if q is None else C.c_void_p(q)
        la = _f3(lobe_a)
        check(lib().vrt_probe_irradiance_device(self.h, vp(d_isects_ptr), int(n), ptr(la, _ffi.f32p), float(lobe_s),
                                                vp(d_rgb_ptr), vp(d_count_ptr), vp(stream_ptr)),
              "vrt_probe_irradiance_device")

    def ray_march(self, rays, even_invisible=False):
        """Batched gi::ray_march over (n, 8) rays {o, d, tmin, tmax} (d
        normalised).  even_invisible: the reference's last parameter -- on a
        scene with probes they are tested too, and a probe hit has tri = ntri +
        k (vrt_ray_march_batch_ex)."""
        rays = np.ascontiguousarray(np.asarray(rays, np.float32).reshape(-1, 8))
        n = rays.shape[0]
        out = np.zeros((max(n, 1), 9), np.uint32)
        if even_invisible:
            check(lib().vrt_ray_march_batch_ex(self.h, rays.ctypes.data_as(C.POINTER(_ffi.Ray)), n,
                                               _ffi.VRT_MARCH_EVEN_INVISIBLE,
                                               out.ctypes.data_as(C.POINTER(_ffi.Hit))),
                  "vrt_ray_march_batch_ex")
        else:
            check(lib().vrt_ray_march_batch(self.h, rays.ctypes.data_as(C.POINTER(_ffi.Ray)), n,
                                            out.ctypes.data_as(C.POINTER(_ffi.Hit))),
                  "vrt_ray_march_batch")
        out = out[:n]
        return {"hit": out[:, 0].astype(np.int32), "tri": out[:, 1].view(np.int32).copy(),
                "voxel": out[:, 2].copy(), "hit_p": out[:, 3:6].view(np.float32).copy(),
                "normal": out[:, 6:9].view(np.float32).copy()}

    def render(self, cam, film, samples=False, counters=False, out=None):
        """Primary render -> (ny, nx, 3) float32 image (+ per-sample dict).
        out: a C-contiguous (ny, nx, 3) float32 array to render into (a film
        reused across frames, as the reference's Film is)."""
        nx, ny = film.nx, film.ny
        if out is not None:
            assert out.shape == (ny, nx, 3) and out.dtype == np.float32 and out.flags.c_contiguous
            rgb = out
        else:
            rgb = np.zeros((ny, nx, 3), np.float32)
        smp = None
        st = None
        so = None
        if samples or counters:
            ns = nx * ny * 4
            so = {}
            s = _ffi.Samples()
            if samples:
                so["hit"] = np.zeros(ns, np.int32)
                so["tri"] = np.zeros(ns, np.int32)
                so["voxel"] = np.zeros(ns, np.uint32)
                so["rgb"] = np.zeros((ns, 3), np.float32)
                s.hit = ptr(so["hit"], _ffi.i32p)
                s.tri = ptr(so["tri"], _ffi.i32p)
                s.voxel = ptr(so["voxel"], _ffi.u32p)
                s.rgb = ptr(so["rgb"], _ffi.f32p)
            if counters:
                so["counters"] = np.zeros((ns, 4), np.uint32)
                s.counters = ptr(so["counters"], _ffi.u32p)
                st = _ffi.Stats()
            smp = C.byref(s)
        check(lib().vrt_render(self.h, C.byref(cam.c), C.byref(film.c), ptr(rgb, _ffi.f32p), smp,
                               C.byref(st) if st is not None else None), "vrt_render")
        if so is not None and st is not None:
            so["stats"] = {"rays": st.rays, "aabb_tests": st.aabb_tests, "leaves": st.leaves,
                           "tri_tests": st.tri_tests, "hits": st.hits, "kernel_ms": st.kernel_ms}
        return (rgb, so) if so is not None else rgb

    def render_secondary(self, cam, film, spp=64, ids=False):
        """Config 5: per-pixel sky visibility from `spp` stochastic secondary
        rays -> (ny, nx) float32 image, rays traced (+ per-ray id dict).
        ids=True: per-ray hit, triangle and voxel ids (the ordered walk);
        ids="hit": per-ray hit booleans only (the occlusion walk with its
        compaction, as without ids)."""
        nx, ny = film.nx, film.ny
        vis = np.zeros((ny, nx), np.float32)
        rays = C.c_int64()
        d = None
        if ids:
            ns = nx * ny * spp
            d = {"hit": np.zeros(ns, np.int32)}
            if ids != "hit":
                d.update(tri=np.zeros(ns, np.int32), voxel=np.zeros(ns, np.uint32))
        check(lib().vrt_render_secondary(self.h, C.byref(cam.c), C.byref(film.c), int(spp), ptr(vis, _ffi.f32p),
                                         ptr(d["hit"], _ffi.i32p) if d else None,
                                         ptr(d["tri"], _ffi.i32p) if d and "tri" in d else None,
                                         ptr(d["voxel"], _ffi.u32p) if d and "voxel" in d else None,
                                         C.byref(rays)),
              "vrt_render_secondary")
        return (vis, rays.value, d) if ids else (vis, rays.value)

    def render_secondary_device(self, cam, film, spp, rank, nranks, d_prim_ptr, d_vis_ptr, stream_ptr=None):
        check(lib().vrt_render_secondary_device(self.h, C.byref(cam.c), C.byref(film.c), int(spp), int(rank),
                                                int(nranks), C.c_void_p(d_prim_ptr), C.c_void_p(d_vis_ptr),
                                                C.c_void_p(stream_ptr) if stream_ptr else None),
              "vrt_render_secondary_device")

    def render_secondary_tiles_device(self, cam, film, spp, rank, nranks, d_prim_ptr, d_vis_ptr, d_packed_ptr,
                                      d_prim_hits_ptr=None, stream_ptr=None):
        """One rank's config-5 share, packed for the gather
        (vrt_render_secondary_tiles_device): the primary pass marches only the
        rank's own tiles; d_packed receives its tiles of the visibility image
        in deal order (64 floats each), d_prim_hits (a device uint64, or
        None) the number of its pixels whose primary ray hit."""
        check(lib().vrt_render_secondary_tiles_device(self.h, C.byref(cam.c), C.byref(film.c), int(spp), int(rank),
                                                      int(nranks), C.c_void_p(d_prim_ptr), C.c_void_p(d_vis_ptr),
                                                      C.c_void_p(d_packed_ptr),
                                                      C.c_void_p(d_prim_hits_ptr) if d_prim_hits_ptr else None,
                                                      C.c_void_p(stream_ptr) if stream_ptr else None),
              "vrt_render_secondary_tiles_device")

    def render_tiles_device(self, cam, film, rank, nranks, image_layout, d_out_ptr, stream_ptr=None):
        check(lib().vrt_render_tiles_device(self.h, C.byref(cam.c), C.byref(film.c), int(rank),
                                            int(nranks), int(image_layout), C.c_void_p(d_out_ptr),
                                            C.c_void_p(stream_ptr) if stream_ptr else None),
              "vrt_render_tiles_device")

    def set_frames_in_flight(self, n):
        """Launch hint (vrt_scene_set_frames_in_flight): n >= 2 frames kept
        in flight on different streams -> half-chip persistent grids."""
        check(lib().vrt_scene_set_frames_in_flight(self.h, int(n)), "vrt_scene_set_frames_in_flight")

    def beam_entries(self):
        """The beam-entry records of the last persistent primary render
        (vrt_debug_beam_entries): uint32 [units, 16], or None when there was
        none."""
        n = C.c_int64()
        check(lib().vrt_debug_beam_entries(self.h, None, 0, C.byref(n)), "vrt_debug_beam_entries")
        if n.value <= 0:
            return None
        out = np.zeros((n.value, 16), np.uint32)
        check(lib().vrt_debug_beam_entries(self.h, out.ctypes.data_as(_ffi.u32p), n.value, C.byref(n)),
              "vrt_debug_beam_entries")
        return out

    def secondary_spill_counts(self):
        """Records appended to each config-5 compaction queue (phase A, resume
        rounds 1..3) by the last secondary launch (vrt_secondary_spill_counts)."""
        c = (C.c_int64 * 4)()
        check(lib().vrt_secondary_spill_counts(self.h, c), "vrt_secondary_spill_counts")
        return list(c)

    def secondary_spill_stats(self):
        """The last config-5 launch's compaction (vrt_secondary_spill_stats):
        {records, finished_in_place, chunks_taken, chunks_allocated,
        leftover_chunks, record_bytes, deferred_pixels}."""
        c = (C.c_int64 * 7)()
        check(lib().vrt_secondary_spill_stats(self.h, c), "vrt_secondary_spill_stats")
        return dict(zip(("records", "finished_in_place", "chunks_taken", "chunks_allocated", "leftover_chunks",
                         "record_bytes", "deferred_pixels"), list(c)))

    def scratch_bytes(self):
        """(total, compaction) device bytes of scratch the scene keeps between
        calls (vrt_scene_scratch_bytes)."""
        t, sp = C.c_int64(), C.c_int64()
        check(lib().vrt_scene_scratch_bytes(self.h, C.byref(t), C.byref(sp)), "vrt_scene_scratch_bytes")
        return t.value, sp.value

    def last_kernel_ms(self):
        ms = C.c_float()
        check(lib().vrt_last_kernel_ms(self.h, C.byref(ms)), "vrt_last_kernel_ms")
        return ms.value

    # ---- full trace() ----
    def min_voxel(self, levels=0):
        """The reference's Res: min(root.size() / 2^levels) (VRT/main.cc:69-70)."""
        r = C.c_float()
        check(lib().vrt_scene_min_voxel(self.h, int(levels), C.byref(r)), "vrt_scene_min_voxel")
        return r.value

    def lightmap(self, light_cam, light_film):
        """Light pass + cone_trace_init_filter on the device; returns hit samples."""
        h = C.c_int64()
        check(lib().vrt_lightmap_build(self.h, C.byref(light_cam.c), C.byref(light_film.c), C.byref(h)),
              "vrt_lightmap_build")
        return h.value

    def lightmap_lights(self, lights):
        """Several coloured lights into one light map
        (vrt_lightmap_build_lights): the light pass run light after light in
        the order given, one filter; returns the hit samples of all lights."""
        arr, n = _lights_arg(lights)
        h = C.c_int64()
        check(lib().vrt_lightmap_build_lights(self.h, arr, n, C.byref(h)), "vrt_lightmap_build_lights")
        return h.value

    def lightmap_nodes(self):
        """(key depth<<32|vox, coverage, illum (n,6,3)) sorted by key."""
        n = self.info.nodes
        key = np.zeros(n, np.uint64)
        cov = np.zeros(n, np.float32)
        ill = np.zeros((n, 6, 3), np.float32)
        check(lib().vrt_lightmap_nodes(self.h, key.ctypes.data_as(C.POINTER(C.c_uint64)), ptr(cov, _ffi.f32p),
                                       ptr(ill, _ffi.f32p)), "vrt_lightmap_nodes")
        o = np.argsort(key, kind="stable")
        return key[o], cov[o], ill[o]

    def lightmap_stats(self):
        """The last light-map build (vrt_lightmap_stats): {samples, hits,
        deferred: samples handed to the tail walk}."""
        c = (C.c_int64 * 3)()
        check(lib().vrt_lightmap_stats(self.h, c), "vrt_lightmap_stats")
        return dict(zip(("samples", "hits", "deferred"), list(c)))

    def render_trace(self, cam, film, min_voxel=0.0, samples=False):
        """trace() render (cone tracing) -> (ny, nx, 3) [+ per-sample hit / rgb]."""
        rgb = np.zeros((film.ny, film.nx, 3), np.float32)
        ns = film.nx * film.ny * 4
        hit = np.zeros(ns, np.int32) if samples else None
        srgb = np.zeros((ns, 3), np.float32) if samples else None
        check(lib().vrt_render_trace(self.h, C.byref(cam.c), C.byref(film.c), float(min_voxel), ptr(rgb, _ffi.f32p),
                                     ptr(hit, _ffi.i32p), ptr(srgb, _ffi.f32p)), "vrt_render_trace")
        return (rgb, {"hit": hit, "rgb": srgb}) if samples else rgb

    def render_trace_device(self, cam, film, rank, nranks, image_layout, d_out_ptr, min_voxel=0.0,
                            stream_ptr=None):
        check(lib().vrt_render_trace_device(self.h, C.byref(cam.c), C.byref(film.c), float(min_voxel), int(rank),
                                            int(nranks), int(image_layout), C.c_void_p(d_out_ptr),
                                            None if stream_ptr is None else C.c_void_p(stream_ptr)),
              "vrt_render_trace_device")

    def trace_frame_device(self, light_cam, light_film, cam, film, rank, nranks, image_layout, d_out_ptr,
                           min_voxel=0.0, stream_ptr=None):
        """The reference main() frame in one call (vrt_trace_frame_device):
        light map + filter beside the view's primary march, then the cones;
        returns the light pass's hit count."""
        hits = C.c_int64()
        check(lib().vrt_trace_frame_device(self.h, C.byref(light_cam.c), C.byref(light_film.c), C.byref(cam.c),
                                           C.byref(film.c), float(min_voxel), int(rank), int(nranks),
                                           int(image_layout), C.c_void_p(d_out_ptr),
                                           None if stream_ptr is None else C.c_void_p(stream_ptr), C.byref(hits)),
              "vrt_trace_frame_device")
        return hits.value

    def trace_frame_lights_device(self, lights, cam, film, rank, nranks, image_layout, d_out_ptr, min_voxel=0.0,
                                  probe_light_color=None, stream_ptr=None):
        """trace_frame_device over a light list (vrt_trace_frame_lights_device).
        probe_light_color is not a light's colour: on a probe scene it is what
        the probes' gather adds on a miss (None keeps the stored SGs).
        Returns the hit samples of all lights."""
        arr, n = _lights_arg(lights)
        hits = C.c_int64()
        lc = None if probe_light_color is None else _f3(probe_light_color)
        check(lib().vrt_trace_frame_lights_device(self.h, arr, n, ptr(lc, _ffi.f32p), C.byref(cam.c), C.byref(film.c),
                                                  float(min_voxel), int(rank), int(nranks), int(image_layout),
                                                  C.c_void_p(d_out_ptr),
                                                  None if stream_ptr is None else C.c_void_p(stream_ptr),
                                                  C.byref(hits)), "vrt_trace_frame_lights_device")
        return hits.value

    # ---- trace() frames of a probe scene (probe hits shaded on the device) ----
    def render_trace_probes(self, cam, film, min_voxel=0.0, samples=False):
        """render_trace on a probe scene (vrt_render_trace_probes): the mixed
        march; samples' hit is 0 miss / 1 triangle / 2 probe."""
        rgb = np.zeros((film.ny, film.nx, 3), np.float32)
        ns = film.nx * film.ny * 4
        hit = np.zeros(ns, np.int32) if samples else None
        srgb = np.zeros((ns, 3), np.float32) if samples else None
        check(lib().vrt_render_trace_probes(self.h, C.byref(cam.c), C.byref(film.c), float(min_voxel),
                                            ptr(rgb, _ffi.f32p), ptr(hit, _ffi.i32p), ptr(srgb, _ffi.f32p)),
              "vrt_render_trace_probes")
        return (rgb, {"hit": hit, "rgb": srgb}) if samples else rgb

    def render_trace_probes_device(self, cam, film, rank, nranks, image_layout, d_out_ptr, min_voxel=0.0,
                                   stream_ptr=None):
        check(lib().vrt_render_trace_probes_device(self.h, C.byref(cam.c), C.byref(film.c), float(min_voxel),
                                                   int(rank), int(nranks), int(image_layout), C.c_void_p(d_out_ptr),
                                                   None if stream_ptr is None else C.c_void_p(stream_ptr)),
              "vrt_render_trace_probes_device")

    def trace_frame_probes_device(self, light_cam, light_film, light_color, cam, film, rank, nranks, image_layout,
                                  d_out_ptr, min_voxel=0.0, stream_ptr=None):
        """The reference main() frame with its probe block in one call
        (vrt_trace_frame_probes_device): light map + filter beside the view's
        mixed march, the scene's probes' gather (light_color None: the stored
        SGs are kept), then the cones and the probe hits' colours; returns the
        light pass's hit count."""
        hits = C.c_int64()
        lc = None if light_color is None else _f3(light_color)
        check(lib().vrt_trace_frame_probes_device(self.h, C.byref(light_cam.c), C.byref(light_film.c),
                                                  ptr(lc, _ffi.f32p), C.byref(cam.c), C.byref(film.c),
                                                  float(min_voxel), int(rank), int(nranks), int(image_layout),
                                                  C.c_void_p(d_out_ptr),
                                                  None if stream_ptr is None else C.c_void_p(stream_ptr),
                                                  C.byref(hits)), "vrt_trace_frame_probes_device")
        return hits.value

    # ---- batched trace() / cone_trace over the caller's rays and points ----
    def trace(self, rays, min_voxel=0.0, parts=False):
        """Batched trace(root, ray, 5, true) (VRT/main.cc:10-30) over (n, 8) rays
        {o, d, tmin, tmax}, taken as they are -> rgb (n, 3).  parts=True also
        returns a dict: ray_march's hit / tri / voxel / hit_p / normal and the
        terms indirect (cone_trace), direct (compute_illum(-d)) and albedo
        (all +0 on a miss; rgb = albedo * (indirect + direct))."""
        rays = np.asarray(rays, np.float32)
        if rays.ndim != 2 or rays.shape[1] != 8:
            raise ValueError(f"rays must be (n, 8) {{o, d, tmin, tmax}}, got {rays.shape}")
        rays = np.ascontiguousarray(rays)
        n = rays.shape[0]
        rgb = np.zeros((n, 3), np.float32)
        pc, hits, ind, dr, alb = None, None, None, None, None
        if parts:
            hits = np.zeros((n, 9), np.uint32)
            ind, dr, alb = (np.zeros((n, 3), np.float32) for _ in range(3))
            pc = _ffi.TraceParts(hits.ctypes.data, ind.ctypes.data, dr.ctypes.data, alb.ctypes.data)
        check(lib().vrt_trace_batch(self.h, rays.ctypes.data_as(C.POINTER(_ffi.Ray)), n, float(min_voxel),
                                    ptr(rgb, _ffi.f32p), None if pc is None else C.byref(pc)),
              "vrt_trace_batch")
        if not parts:
            return rgb
        return rgb, {"hit": hits[:, 0].astype(np.int32), "tri": hits[:, 1].view(np.int32).copy(),
                     "voxel": hits[:, 2].copy(), "hit_p": hits[:, 3:6].view(np.float32).copy(),
                     "normal": hits[:, 6:9].view(np.float32).copy(), "indirect": ind, "direct": dr,
                     "albedo": alb}

    def cone_trace(self, hit_p, normal, min_voxel=0.0):
        """Batched gi::cone_trace(root, isect, min_voxel) (VRT/voxel_octree.cc:
        313-330) at (n, 3) points with (n, 3) normals -> (n, 3)."""
        hit_p, normal = np.asarray(hit_p, np.float32), np.asarray(normal, np.float32)
        if hit_p.ndim != 2 or hit_p.shape[1] != 3 or normal.shape != hit_p.shape:
            raise ValueError(f"hit_p and normal must both be (n, 3), got {hit_p.shape} and {normal.shape}")
        isects = np.ascontiguousarray(np.concatenate([hit_p, normal], axis=1))
        n = isects.shape[0]
        rgb = np.zeros((n, 3), np.float32)
        check(lib().vrt_cone_trace_batch(self.h, isects.ctypes.data_as(C.POINTER(_ffi.ISect)), n,
                                         float(min_voxel), ptr(rgb, _ffi.f32p)), "vrt_cone_trace_batch")
        return rgb

    def trace_device(self, d_rays_ptr, n, d_rgb_ptr, min_voxel=0.0, d_hits_ptr=None, d_indirect_ptr=None,
                     d_direct_ptr=None, d_albedo_ptr=None, stream_ptr=None):
        """vrt_trace_batch_device: raw device pointers (n vrt_ray in, 3n floats
        out, optional vrt_hit / 3n-float parts), enqueued on the stream."""
        pc = _ffi.TraceParts(d_hits_ptr, d_indirect_ptr, d_direct_ptr, d_albedo_ptr)
        check(lib().vrt_trace_batch_device(self.h, C.c_void_p(d_rays_ptr), int(n), float(min_voxel),
                                           C.c_void_p(d_rgb_ptr), C.byref(pc),
                                           None if stream_ptr is None else C.c_void_p(stream_ptr)),
              "vrt_trace_batch_device")

    def cone_trace_device(self, d_isects_ptr, n, d_rgb_ptr, min_voxel=0.0, stream_ptr=None):
        """vrt_cone_trace_batch_device: n vrt_isect {hit_p, normal} in, 3n floats out."""
        check(lib().vrt_cone_trace_batch_device(self.h, C.c_void_p(d_isects_ptr), int(n), float(min_voxel),
                                                C.c_void_p(d_rgb_ptr),
                                                None if stream_ptr is None else C.c_void_p(stream_ptr)),
              "vrt_cone_trace_batch_device")

    # ---- light probes (LightProbe::gather_light, batched) ----
    def probe_gather(self, probes, min_voxel=0.0, light_color=(1.0, 1.0, 1.0), points=None, terms=False):
        """LightProbe::gather_light (VRT/voxel_octree.cc:592-618) for (n, 4)
        probes {o, r} -> SGs as a dict a (n, 14, 3), d (n, 14, 3), s (n, 14).
        points: (npoints, 3) sample points of the caller's (None: the
        reference's 100).  terms=True also returns (n, 14, npoints, 3): what
        each ray added to litness."""
        probes = np.asarray(probes, np.float32)
        if probes.ndim != 2 or probes.shape[1] != 4:
            raise ValueError(f"probes must be (n, 4) {{o, r}}, got {probes.shape}")
        probes = np.ascontiguousarray(probes)
        pts, npts = _probe_points_arg(points)
        lc = _f3(light_color)
        n = probes.shape[0]
        sgs = np.zeros((n, PROBE_SGS, 7), np.float32)
        tm = np.zeros((n, PROBE_SGS, npts, 3), np.float32) if terms else None
        check(lib().vrt_probe_gather(self.h, probes.ctypes.data_as(C.POINTER(_ffi.Probe)), n, float(min_voxel),
                                     ptr(lc, _ffi.f32p), ptr(pts, _ffi.f32p), npts if pts is not None else 0,
                                     sgs.ctypes.data_as(C.POINTER(_ffi.SGRec)), ptr(tm, _ffi.f32p)),
              "vrt_probe_gather")
        out = {"a": sgs[:, :, 0:3].copy(), "d": sgs[:, :, 3:6].copy(), "s": sgs[:, :, 6].copy()}
        return (out, tm) if terms else out

    def probe_gather_device(self, d_probes_ptr, n, d_sgs_ptr, min_voxel=0.0, light_color=(1.0, 1.0, 1.0),
                            points=None, d_terms_ptr=None, stream_ptr=None):
        """vrt_probe_gather_device: raw device pointers (n vrt_probe in, 14 n
        vrt_sg out, optional 3 * 14 * npoints * n floats of terms), enqueued
        on the stream; points stays a host array."""
        pts, npts = _probe_points_arg(points)
        lc = _f3(light_color)
        check(lib().vrt_probe_gather_device(self.h, C.c_void_p(d_probes_ptr), int(n), float(min_voxel),
                                            ptr(lc, _ffi.f32p), ptr(pts, _ffi.f32p),
                                            npts if pts is not None else 0, C.c_void_p(d_sgs_ptr),
                                            None if d_terms_ptr is None else C.c_void_p(d_terms_ptr),
                                            None if stream_ptr is None else C.c_void_p(stream_ptr)),
              "vrt_probe_gather_device")


class MultiOctree:
    """The octree replicated on every device of a mask, with an RCCL
    communicator over them (vrt_scene_create_multi): one frame = every
    device's share of the tile deal + one ncclGather to the first device +
    unpack there -- render_mt (VRT/camera.h:42-68) over a node's GPUs."""

    def __init__(self, scene, max_depth, device_mask=1, build_on_device=False, virtual_ranks=None, probes=None,
                 light_mode="replicated"):
        """virtual_ranks=n (test hook, VRT_TEST_VIRTUAL_RANKS_N): n ranks on
        the one device of device_mask, the RCCL gather replaced by
        device-to-device copies -- the n-rank frame on a one-GPU box.
        probes: as VoxelOctree's (vrt_scene_create_multi_probes); every rank
        holds the same probe scene.  light_mode: "replicated" (every rank
        marches the whole light film) or "sharded" (each its tiles of the
        light film's deal, hit lists exchanged), see light_mode."""
        self.scene_data = scene  # keeps the arrays alive for the descriptor
        h = C.c_void_p()
        d = scene.desc()
        flags = _ffi.VRT_BUILD_DEVICE if build_on_device else 0
        self.probes = _probes_arg(probes)
        if build_on_device and self.probes is not None:
            flags |= _ffi.VRT_BUILD_DEVICE_PROBES

        def create():
            if self.probes is None:
                return lib().vrt_scene_create_multi(C.byref(d), int(max_depth), int(device_mask), flags, C.byref(h))
            return lib().vrt_scene_create_multi_probes(C.byref(d), self.probes.ctypes.data_as(C.POINTER(_ffi.Probe)),
                                                       len(self.probes), int(max_depth), int(device_mask), flags,
                                                       C.byref(h))
        if virtual_ranks:
            prev = lib().vrt_test_flags()  # restored afterwards: a caller's own test flags stay set
            lib().vrt_set_test_flags((prev & 0xFF & ~TEST_VIRTUAL_RANKS) | TEST_VIRTUAL_RANKS
                                     | (int(virtual_ranks) << 8))
            try:
                rc = create()
            finally:
                lib().vrt_set_test_flags(prev)
        else:
            rc = create()
        check(rc, "vrt_scene_create_multi")
        self.h = h
        n = C.c_int32()
        check(lib().vrt_multi_devices(self.h, C.byref(n), None), "vrt_multi_devices")
        devs = np.zeros(n.value, np.int32)
        check(lib().vrt_multi_devices(self.h, C.byref(n), ptr(devs, _ffi.i32p)), "vrt_multi_devices")
        self.devices = [int(x) for x in devs]
        s0 = C.c_void_p()
        check(lib().vrt_multi_scene(self.h, 0, C.byref(s0)), "vrt_multi_scene")
        self.info = _ffi.SceneInfo()
        check(lib().vrt_scene_info(s0, C.byref(self.info)), "vrt_scene_info")
        self.max_depth = int(max_depth)
        self._light_mode = "replicated"
        self.light_mode = light_mode

    def close(self):
        if self.h:
            lib().vrt_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def root_box(self):
        return (np.array(self.info.root_min[:], np.float32), np.array(self.info.root_max[:], np.float32))

    def render(self, cam, film):
        """The whole frame -> (ny, nx, 3) float32 host image."""
        rgb = np.zeros((film.ny, film.nx, 3), np.float32)
        check(lib().vrt_render_multi(self.h, C.byref(cam.c), C.byref(film.c), ptr(rgb, _ffi.f32p)),
              "vrt_render_multi")
        return rgb

    def render_device(self, cam, film, d_image_ptr, stream_ptr=None):
        """The whole frame into a device image on the first device."""
        check(lib().vrt_render_multi_device(self.h, C.byref(cam.c), C.byref(film.c), C.c_void_p(d_image_ptr),
                                            C.c_void_p(stream_ptr) if stream_ptr else None),
              "vrt_render_multi_device")

    def render_secondary(self, cam, film, spp=64):
        """Config 5 over the handle's ranks (vrt_render_secondary_multi) ->
        ((ny, nx) float32 visibility image, rays traced): VoxelOctree's
        render_secondary, bit for bit, for any rank count."""
        vis = np.zeros((film.ny, film.nx), np.float32)
        rays = C.c_int64()
        check(lib().vrt_render_secondary_multi(self.h, C.byref(cam.c), C.byref(film.c), int(spp),
                                               ptr(vis, _ffi.f32p), C.byref(rays)), "vrt_render_secondary_multi")
        return vis, rays.value

    def render_secondary_device(self, cam, film, spp, d_vis_ptr, stream_ptr=None):
        """render_secondary into a device image (nx*ny floats) on the first
        device, ordered on stream_ptr as render_device is."""
        check(lib().vrt_render_secondary_multi_device(self.h, C.byref(cam.c), C.byref(film.c), int(spp),
                                                      C.c_void_p(d_vis_ptr),
                                                      C.c_void_p(stream_ptr) if stream_ptr else None),
              "vrt_render_secondary_multi_device")

    # ---- moving geometry ----
    def _update_done(self, probes):
        if probes is not None:
            self.probes = probes
        s0 = C.c_void_p()
        check(lib().vrt_multi_scene(self.h, 0, C.byref(s0)), "vrt_multi_scene")
        check(lib().vrt_scene_info(s0, C.byref(self.info)), "vrt_scene_info")

    def update(self, pos, nrm=None, probes=None, verify=False):
        """Rebuild every rank's scene in place from new vertex positions
        (ntri*9 floats), unless nrm is None new normals, and on a probe handle
        unless probes is None new probes (vrt_multi_update).  All ranks or
        none: a refusal raises and leaves every rank on its previous geometry.
        verify: compare the ranks' digests afterwards."""
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1)
        n9 = 9 * self.scene_data.ntri
        if pos.size != n9:
            raise ValueError(f"pos has {pos.size} floats, the scene needs {n9}")
        if nrm is not None:
            nrm = np.ascontiguousarray(nrm, np.float32).reshape(-1)
            if nrm.size != n9:
                raise ValueError(f"nrm has {nrm.size} floats, the scene needs {n9}")
        pp = None
        if probes is not None:
            probes = _probes_arg(probes)
            have = 0 if self.probes is None else len(self.probes)
            if probes is None:
                raise ValueError("probes is empty")
            if have and len(probes) != have:
                raise ValueError(f"probes has {len(probes)} records, the handle has {have}")
            pp = probes.ctypes.data_as(C.POINTER(_ffi.Probe))
        check(lib().vrt_multi_update(self.h, ptr(pos, _ffi.f32p), ptr(nrm, _ffi.f32p), pp,
                                     _ffi.VRT_MULTI_UPDATE_VERIFY if verify else 0), "vrt_multi_update")
        self._update_done(probes)

    def update_device(self, d_pos_ptr, d_nrm_ptr=None, d_probes_ptr=None, stream_ptr=None, verify=False):
        """update() from arrays on the first device, read in the order of
        stream_ptr (vrt_multi_update_device); every rank is ready on return."""
        check(lib().vrt_multi_update_device(self.h, C.c_void_p(d_pos_ptr),
                                            C.c_void_p(d_nrm_ptr) if d_nrm_ptr else None,
                                            C.c_void_p(d_probes_ptr) if d_probes_ptr else None,
                                            _ffi.VRT_MULTI_UPDATE_VERIFY if verify else 0,
                                            C.c_void_p(stream_ptr) if stream_ptr else None),
              "vrt_multi_update_device")
        self._update_done(self.scene(0).device_array(7).view(np.float32).reshape(-1, 4).copy()
                          if d_probes_ptr else None)

    def update_stats(self):
        """The last update's wall-clock split in ms (vrt_multi_update_stats)."""
        ms = np.zeros(4, np.float64)
        check(lib().vrt_multi_update_stats(self.h, ptr(ms, _ffi.f64p)), "vrt_multi_update_stats")
        return dict(total=ms[0], slowest_rank=ms[1], distribute=ms[2], verify=ms[3])

    # ---- trace() frames (light pass + filter + cone-traced view) ----
    LIGHT_MODES = {"replicated": _ffi.VRT_MULTI_LIGHT_REPLICATED, "sharded": _ffi.VRT_MULTI_LIGHT_SHARDED}

    @property
    def light_mode(self):
        """How the ranks share a light-map build (vrt_multi_set_light_mode):
        "replicated" or "sharded"; the light map is the same bits either way."""
        return self._light_mode

    @light_mode.setter
    def light_mode(self, mode):
        check(lib().vrt_multi_set_light_mode(self.h, self.LIGHT_MODES.get(mode, -1) if isinstance(mode, str)
                                             else int(mode)), "vrt_multi_set_light_mode")
        self._light_mode = mode if isinstance(mode, str) else {v: k for k, v in self.LIGHT_MODES.items()}[int(mode)]

    def scene(self, rank):
        """Rank `rank`'s scene (vrt_multi_scene) as a VoxelOctree that borrows
        the handle's: lightmap_nodes(), lightmap_stats(), probe_sgs, ..."""
        s = C.c_void_p()
        check(lib().vrt_multi_scene(self.h, int(rank), C.byref(s)), "vrt_multi_scene")
        return _RankScene(self, s)

    def min_voxel(self, levels=0):
        return self.scene(0).min_voxel(levels)

    @property
    def probe_sgs(self):
        """Rank 0's stored SGs (every rank holds the same)."""
        return self.scene(0).probe_sgs

    @probe_sgs.setter
    def probe_sgs(self, sgs):
        """The stored SGs of every rank (vrt_multi_set_probe_sgs)."""
        n = self.scene(0).probe_info()[0]
        a, d, s = (np.asarray(sgs[k], np.float32) for k in ("a", "d", "s"))
        if a.shape != (n, PROBE_SGS, 3) or d.shape != a.shape or s.shape != (n, PROBE_SGS):
            raise ValueError(f"sgs must hold a, d ({n}, 14, 3) and s ({n}, 14), got {a.shape}, {d.shape}, {s.shape}")
        rec = np.ascontiguousarray(np.concatenate([a, d, s[:, :, None]], axis=2))
        check(lib().vrt_multi_set_probe_sgs(self.h, rec.ctypes.data_as(C.POINTER(_ffi.SGRec))),
              "vrt_multi_set_probe_sgs")

    def lightmap(self, light_cam, light_film):
        """The light map on every rank (vrt_lightmap_build_multi); returns the
        light pass's hit count."""
        h = C.c_int64()
        check(lib().vrt_lightmap_build_multi(self.h, C.byref(light_cam.c), C.byref(light_film.c), C.byref(h)),
              "vrt_lightmap_build_multi")
        return h.value

    def lightmap_lights(self, lights):
        """Several coloured lights into one light map on every rank
        (vrt_lightmap_build_lights_multi); returns the hits of all lights."""
        arr, n = _lights_arg(lights)
        h = C.c_int64()
        check(lib().vrt_lightmap_build_lights_multi(self.h, arr, n, C.byref(h)), "vrt_lightmap_build_lights_multi")
        return h.value

    def trace_frame_lights(self, lights, cam, film, min_voxel=0.0, probe_light_color=None):
        """trace_frame over a light list (vrt_trace_frame_lights_multi) ->
        ((ny, nx, 3) image, hits of all lights).  probe_light_color: the
        probes' gather's miss colour on a probe handle, not a light's colour."""
        arr, n = _lights_arg(lights)
        rgb = np.zeros((film.ny, film.nx, 3), np.float32)
        h = C.c_int64()
        lc = None if probe_light_color is None else _f3(probe_light_color)
        check(lib().vrt_trace_frame_lights_multi(self.h, arr, n, ptr(lc, _ffi.f32p), C.byref(cam.c), C.byref(film.c),
                                                 float(min_voxel), ptr(rgb, _ffi.f32p), C.byref(h)),
              "vrt_trace_frame_lights_multi")
        return rgb, h.value

    def trace_frame_lights_device(self, lights, cam, film, d_image_ptr, min_voxel=0.0, probe_light_color=None,
                                  stream_ptr=None):
        """trace_frame_lights into a device image on the first device."""
        arr, n = _lights_arg(lights)
        h = C.c_int64()
        lc = None if probe_light_color is None else _f3(probe_light_color)
        check(lib().vrt_trace_frame_lights_multi_device(self.h, arr, n, ptr(lc, _ffi.f32p), C.byref(cam.c),
                                                        C.byref(film.c), float(min_voxel), C.c_void_p(d_image_ptr),
                                                        C.c_void_p(stream_ptr) if stream_ptr else None, C.byref(h)),
              "vrt_trace_frame_lights_multi_device")
        return h.value

    def render_trace(self, cam, film, min_voxel=0.0):
        """The cone-traced view over the ranks' light maps -> (ny, nx, 3)."""
        rgb = np.zeros((film.ny, film.nx, 3), np.float32)
        check(lib().vrt_render_trace_multi(self.h, C.byref(cam.c), C.byref(film.c), float(min_voxel),
                                           ptr(rgb, _ffi.f32p)), "vrt_render_trace_multi")
        return rgb

    def render_trace_device(self, cam, film, d_image_ptr, min_voxel=0.0, stream_ptr=None):
        check(lib().vrt_render_trace_multi_device(self.h, C.byref(cam.c), C.byref(film.c), float(min_voxel),
                                                  C.c_void_p(d_image_ptr),
                                                  C.c_void_p(stream_ptr) if stream_ptr else None),
              "vrt_render_trace_multi_device")

    def trace_frame(self, light_cam, light_film, cam, film, min_voxel=0.0, light_color=None):
        """The reference main() frame (vrt_trace_frame_multi) -> ((ny, nx, 3)
        image, light hits).  light_color: on a probe handle, gather the probes
        behind the filter on every rank (None keeps the stored SGs)."""
        rgb = np.zeros((film.ny, film.nx, 3), np.float32)
        h = C.c_int64()
        lc = None if light_color is None else _f3(light_color)
        check(lib().vrt_trace_frame_multi(self.h, C.byref(light_cam.c), C.byref(light_film.c), ptr(lc, _ffi.f32p),
                                          C.byref(cam.c), C.byref(film.c), float(min_voxel), ptr(rgb, _ffi.f32p),
                                          C.byref(h)), "vrt_trace_frame_multi")
        return rgb, h.value

    def trace_frame_device(self, light_cam, light_film, cam, film, d_image_ptr, min_voxel=0.0, light_color=None,
                           stream_ptr=None):
        """trace_frame into a device image on the first device, ordered on
        stream_ptr as render_device is; returns the light pass's hit count."""
        h = C.c_int64()
        lc = None if light_color is None else _f3(light_color)
        check(lib().vrt_trace_frame_multi_device(self.h, C.byref(light_cam.c), C.byref(light_film.c),
                                                 ptr(lc, _ffi.f32p), C.byref(cam.c), C.byref(film.c),
                                                 float(min_voxel), C.c_void_p(d_image_ptr),
                                                 C.c_void_p(stream_ptr) if stream_ptr else None, C.byref(h)),
              "vrt_trace_frame_multi_device")
        return h.value


class _RankScene(VoxelOctree):
    """One rank's scene of a MultiOctree: the handle owns it."""

    def __init__(self, multi, h):
        self.multi = multi  # keeps the handle alive
        self.scene = multi.scene_data
        self.probes = multi.probes
        self.h = h
        self.max_depth = multi.max_depth
        self.info = _ffi.SceneInfo()
        check(lib().vrt_scene_info(self.h, C.byref(self.info)), "vrt_scene_info")

    def close(self):
        self.h = None


def multi_tile_map(film, device_mask):
    """The deal of a frame over a device mask as (nty, ntx) arrays: each
    tile's device and its index in that device's buffer (vrt_multi_tile_map)."""
    ntx, nty = film.nx // 8, film.ny // 8
    dv = np.zeros((nty, ntx), np.int32)
    sl = np.zeros((nty, ntx), np.int32)
    check(lib().vrt_multi_tile_map(C.byref(film.c), int(device_mask), ptr(dv, _ffi.i32p), ptr(sl, _ffi.i32p)),
          "vrt_multi_tile_map")
    return dv, sl


def ray_march_init(scene, max_depth, device=0, probes=None):
    """gi::ray_march_init(root, voxels, max_depth) (VRT/voxel_octree.cc:67-75);
    voxels = the scene's triangles, then `probes` (VRT/main.cc:56-64)."""
    return VoxelOctree(scene, max_depth, device, probes=probes)


def ray_march(tree, rays, even_invisible=False):
    """gi::ray_march over a batch of rays (VRT/voxel_octree.cc:131-188)."""
    return tree.ray_march(rays, even_invisible)


def _probes_arg(probes):
    """None, an (n, 4) array {o, r} or a sequence of LightProbe -> (n, 4) or None."""
    if probes is None:
        return None
    if len(probes) and isinstance(probes[0], LightProbe):
        probes = [np.concatenate([p.o, [p.r]]) for p in probes]
    probes = np.asarray(probes, np.float32)
    if probes.size == 0:
        return None
    if probes.ndim != 2 or probes.shape[1] != 4:
        raise ValueError(f"probes must be (n, 4) {{o, r}}, got {probes.shape}")
    return np.ascontiguousarray(probes)


def trace(tree, rays, min_voxel=0.0, parts=False):
    """The driver's trace(root, ray, 5, true) (VRT/main.cc:10-30), batched."""
    return tree.trace(rays, min_voxel, parts)


def cone_trace(tree, hit_p, normal, min_voxel=0.0):
    """gi::cone_trace(root, isect, min_voxel_size) (VRT/voxel_octree.h), batched."""
    return tree.cone_trace(hit_p, normal, min_voxel)


# ---- light probes (gi::SG, gi::LightProbe; VRT/voxel_octree.h:120-163) ----
PROBE_SGS = 14  # include/vrt.h VRT_PROBE_SGS
# LightProbe::dirs_ (VRT/voxel_octree.h:156-160): the 6 axes, the 8 diagonals
PROBE_DIRS = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1), (1, 1, 1), (1, 1, -1),
                       (1, -1, 1), (1, -1, -1), (-1, 1, 1), (-1, 1, -1), (-1, -1, 1), (-1, -1, -1)], np.float32)


def probe_points(seed=0xc01dbeef, n=100):
    """The sample points LightProbe::LightProbe draws (vrt_probe_points):
    jql::PCG{seed}, n calls of random_point_in_unit_sphere -> (n, 3)."""
    n = int(n)
    pts = np.zeros((max(n, 0), 3), np.float32)
    check(lib().vrt_probe_points(int(seed) & 0xFFFFFFFFFFFFFFFF, n, ptr(pts, _ffi.f32p)), "vrt_probe_points")
    return pts


def _probe_points_arg(points):
    """(array or None, npoints) for the gather calls."""
    if points is None:
        return None, 100
    pts = np.asarray(points, np.float32)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"points must be (npoints, 3), got {pts.shape}")
    return np.ascontiguousarray(pts), pts.shape[0]


def probe_eval(sgs, dirs):
    """LightProbe::eval (vrt_probe_eval): sgs = the dict probe_gather returns
    (a, d (n, 14, 3), s (n, 14)), dirs (m, 3) -> (n, m, 3)."""
    a, d, s = (np.asarray(sgs[k], np.float32) for k in ("a", "d", "s"))
    if a.ndim != 3 or a.shape[1:] != (PROBE_SGS, 3) or d.shape != a.shape or s.shape != a.shape[:2]:
        raise ValueError(f"sgs must hold a, d (n, 14, 3) and s (n, 14), got {a.shape}, {d.shape}, {s.shape}")
    dirs = np.asarray(dirs, np.float32)
    if dirs.ndim != 2 or dirs.shape[1] != 3:
        raise ValueError(f"dirs must be (m, 3), got {dirs.shape}")
    dirs = np.ascontiguousarray(dirs)
    rec = np.ascontiguousarray(np.concatenate([a, d, s[:, :, None]], axis=2))
    n, m = rec.shape[0], dirs.shape[0]
    rgb = np.zeros((n, m, 3), np.float32)
    check(lib().vrt_probe_eval(rec.ctypes.data_as(C.POINTER(_ffi.SGRec)), n, ptr(dirs, _ffi.f32p), m,
                               ptr(rgb, _ffi.f32p)), "vrt_probe_eval")
    return rgb


def probe_eval_device(d_sgs_ptr, n, d_dirs_ptr, m, d_rgb_ptr, device=0, stream_ptr=None):
    """vrt_probe_eval_device: probe_eval over device arrays (14 n vrt_sg
    records, m x 3 directions -> n x m x 3), enqueued on the stream."""
    check(lib().vrt_probe_eval_device(int(device), C.c_void_p(d_sgs_ptr), int(n), C.c_void_p(d_dirs_ptr), int(m),
                                      C.c_void_p(d_rgb_ptr), None if stream_ptr is None else C.c_void_p(stream_ptr)),
          "vrt_probe_eval_device")


def expf_flavour():
    """Which flavour of the expf model this process's C library computes: 1
    (fused reduction), 0 (plain) or -1 (neither: no device shading)."""
    f = C.c_int()
    check(lib().vrt_expf_flavour(C.byref(f)), "vrt_expf_flavour")
    return f.value


def expf_model(x, flavour, device=None):
    """The model of expf over a float32 array: on the host (vrt_expf_model),
    or by the kernels' code on `device` (vrt_expf_model_device)."""
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    if device is None:
        check(lib().vrt_expf_model(ptr(x, _ffi.f32p), x.size, int(flavour), ptr(y, _ffi.f32p)), "vrt_expf_model")
    else:
        check(lib().vrt_expf_model_device(int(device), ptr(x, _ffi.f32p), x.size, int(flavour), ptr(y, _ffi.f32p)),
              "vrt_expf_model_device")
    return y


def expf_selftest(first_bits, count, stride=1, flavour=None, device=-1):
    """vrt_expf_selftest: the model (device < 0: on the host) against libm's
    expf on the bit patterns first_bits + k * stride, k < count -> (mismatches,
    first bad pattern or None)."""
    if flavour is None:
        flavour = expf_flavour()
    bad, first = C.c_uint64(), C.c_uint32()
    check(lib().vrt_expf_selftest(int(device), int(first_bits), int(count), int(stride), int(flavour),
                                  C.byref(bad), C.byref(first)), "vrt_expf_selftest")
    return bad.value, (first.value if bad.value else None)


# ---- the SG algebra (VRT/voxel_octree.cc:497-528), batched ----
def _sg_recs(sgs, what="sgs"):
    """(n, 7) float32 records {a, d, s}, C-contiguous."""
    sgs = np.asarray(sgs, np.float32)
    if sgs.ndim != 2 or sgs.shape[1] != 7:
        raise ValueError(f"{what} must be (n, 7) {{a, d, s}}, got {sgs.shape}")
    return np.ascontiguousarray(sgs)


def _sg_pair(lhs, rhs):
    lhs, rhs = _sg_recs(lhs, "lhs"), _sg_recs(rhs, "rhs")
    if lhs.shape != rhs.shape:
        raise ValueError(f"lhs and rhs must have the same length, got {lhs.shape[0]} and {rhs.shape[0]}")
    return lhs, rhs


def _sgp(a):
    return a.ctypes.data_as(C.POINTER(_ffi.SGRec))


def sg_make(a, d, s):
    """gi::SG's constructor (vrt_sg_make): a, d (n, 3), s (n,) -> (n, 7)
    records {a, d / length(d), s}."""
    a, d = np.asarray(a, np.float32), np.asarray(d, np.float32)
    s = np.ascontiguousarray(np.asarray(s, np.float32).reshape(-1))
    if a.ndim != 2 or a.shape[1] != 3 or d.shape != a.shape or s.shape[0] != a.shape[0]:
        raise ValueError(f"a, d must be (n, 3) and s (n,), got {a.shape}, {d.shape}, {s.shape}")
    a, d = np.ascontiguousarray(a), np.ascontiguousarray(d)
    out = np.zeros((a.shape[0], 7), np.float32)
    check(lib().vrt_sg_make(ptr(a, _ffi.f32p), ptr(d, _ffi.f32p), ptr(s, _ffi.f32p), a.shape[0], _sgp(out)),
          "vrt_sg_make")
    return out


def sg_integral(sgs):
    """SG::integral (vrt_sg_integral): (n, 7) records -> (n, 3)."""
    sgs = _sg_recs(sgs)
    rgb = np.zeros((sgs.shape[0], 3), np.float32)
    check(lib().vrt_sg_integral(_sgp(sgs), sgs.shape[0], ptr(rgb, _ffi.f32p)), "vrt_sg_integral")
    return rgb


def sg_prod(lhs, rhs):
    """gi::prod (vrt_sg_prod), pairwise: (n, 7), (n, 7) -> (n, 7)."""
    lhs, rhs = _sg_pair(lhs, rhs)
    out = np.zeros_like(lhs)
    check(lib().vrt_sg_prod(_sgp(lhs), _sgp(rhs), lhs.shape[0], _sgp(out)), "vrt_sg_prod")
    return out


def sg_inner_prod(lhs, rhs):
    """gi::inner_prod (vrt_sg_inner_prod), pairwise: (n, 7), (n, 7) -> (n, 3)."""
    lhs, rhs = _sg_pair(lhs, rhs)
    rgb = np.zeros((lhs.shape[0], 3), np.float32)
    check(lib().vrt_sg_inner_prod(_sgp(lhs), _sgp(rhs), lhs.shape[0], ptr(rgb, _ffi.f32p)), "vrt_sg_inner_prod")
    return rgb


def _vp(q):
    return None if q is None else C.c_void_p(q)


def sg_integral_device(d_sgs_ptr, n, d_rgb_ptr, device=0, stream_ptr=None):
    """vrt_sg_integral_device: n vrt_sg records in, 3n floats out (device
    pointers), enqueued on the stream."""
    check(lib().vrt_sg_integral_device(int(device), _vp(d_sgs_ptr), int(n), _vp(d_rgb_ptr), _vp(stream_ptr)),
          "vrt_sg_integral_device")


def sg_prod_device(d_lhs_ptr, d_rhs_ptr, n, d_out_ptr, device=0, stream_ptr=None):
    """vrt_sg_prod_device: n + n vrt_sg records in, n out (device pointers)."""
    check(lib().vrt_sg_prod_device(int(device), _vp(d_lhs_ptr), _vp(d_rhs_ptr), int(n), _vp(d_out_ptr),
                                   _vp(stream_ptr)), "vrt_sg_prod_device")


def sg_inner_prod_device(d_lhs_ptr, d_rhs_ptr, n, d_rgb_ptr, device=0, stream_ptr=None):
    """vrt_sg_inner_prod_device: n + n vrt_sg records in, 3n floats out
    (device pointers)."""
    check(lib().vrt_sg_inner_prod_device(int(device), _vp(d_lhs_ptr), _vp(d_rhs_ptr), int(n), _vp(d_rgb_ptr),
                                         _vp(stream_ptr)), "vrt_sg_inner_prod_device")


class SG:
    """gi::SG (VRT/voxel_octree.cc:497-508): amplitude a, axis d (normalised
    by the library when it comes from a gather), sharpness s."""

    def __init__(self, a, d, s):
        self.a, self.d, self.s = _f3(a), _f3(d), np.float32(s)

    def _rec(self):
        return np.concatenate([self.a, self.d, [self.s]]).astype(np.float32)[None, :]

    @classmethod
    def _of(cls, rec):
        return cls(rec[0:3], rec[3:6], rec[6])

    @classmethod
    def make(cls, a, d, s):
        """The reference's constructor SG{a, d, s}: d normalised (vrt_sg_make)."""
        return cls._of(sg_make(_f3(a)[None, :], _f3(d)[None, :], [s])[0])

    def integral(self):
        """SG::integral (VRT/voxel_octree.cc:509-513) -> (3,)."""
        return sg_integral(self._rec())[0]

    def eval(self, dir):
        """a * expf(s * (dot(dir, d) - 1)): one lobe through vrt_probe_eval
        (the other 13 lobes of the record are zero and add +0)."""
        sgs = {"a": np.zeros((1, PROBE_SGS, 3), np.float32), "d": np.zeros((1, PROBE_SGS, 3), np.float32),
               "s": np.zeros((1, PROBE_SGS), np.float32)}
        sgs["a"][0, 0], sgs["d"][0, 0], sgs["s"][0, 0] = self.a, self.d, self.s
        return probe_eval(sgs, _f3(dir)[None, :])[0, 0]


def prod(lhs, rhs):
    """gi::prod(lhs, rhs) (VRT/voxel_octree.cc:514-521) -> SG."""
    return SG._of(sg_prod(lhs._rec(), rhs._rec())[0])


def inner_prod(lhs, rhs):
    """gi::inner_prod(lhs, rhs) (VRT/voxel_octree.cc:522-528) -> (3,)."""
    return sg_inner_prod(lhs._rec(), rhs._rec())[0]


class LightProbe:
    """gi::LightProbe(o, r) (VRT/voxel_octree.cc:530-632): gather_light fills
    the 14 SGs on the GPU (one probe of VoxelOctree.probe_gather; gather many
    probes with that call), eval sums them."""

    def __init__(self, o, r):
        self.o, self.r = _f3(o), np.float32(r)
        self.sgs = None

    def _rec4(self):
        return np.ascontiguousarray(np.concatenate([self.o, [self.r]]).astype(np.float32))

    def get_aabb(self):
        """AABB3D{o_ - r_, o_ + r_} (VRT/voxel_octree.cc:541-544) -> (min, max)."""
        return (self.o - self.r).astype(np.float32), (self.o + self.r).astype(np.float32)

    def is_visible(self):
        """VRT/voxel_octree.cc:588-591."""
        return False

    def is_overlap(self, box_min, box_max):
        """LightProbe::is_overlap (VRT/voxel_octree.cc:567-586), vrt_probe_overlap."""
        box = np.ascontiguousarray(np.concatenate([_f3(box_min), _f3(box_max)]))
        p = self._rec4()
        rc = lib().vrt_probe_overlap(p.ctypes.data_as(C.POINTER(_ffi.Probe)), ptr(box, _ffi.f32p))
        if rc < 0:
            check(rc, "vrt_probe_overlap")
        return rc == 1

    def isect(self, ray, prev_hit=(0.0, 0.0, 0.0)):
        """LightProbe::isect (VRT/voxel_octree.cc:546-554), vrt_probe_isect: ray
        = 8 floats {o, d, tmin, tmax}; prev_hit = the hit point the caller's
        ISect held.  None on a miss, else (t, hit_p, normal)."""
        ray = np.ascontiguousarray(np.asarray(ray, np.float32).reshape(8))
        p, ph = self._rec4(), _f3(prev_hit)
        t, hp, nr = C.c_float(), np.zeros(3, np.float32), np.zeros(3, np.float32)
        rc = lib().vrt_probe_isect(p.ctypes.data_as(C.POINTER(_ffi.Probe)), ray.ctypes.data_as(C.POINTER(_ffi.Ray)),
                                   ptr(ph, _ffi.f32p), C.byref(t), ptr(hp, _ffi.f32p), ptr(nr, _ffi.f32p))
        if rc < 0:
            check(rc, "vrt_probe_isect")
        return (np.float32(t.value), hp, nr) if rc == 1 else None

    def gather_light(self, tree, res, light_color):
        probe = np.concatenate([self.o, [self.r]]).astype(np.float32)[None, :]
        g = tree.probe_gather(probe, res, light_color)
        self._rec = g
        self.sgs = [SG(g["a"][0, i], g["d"][0, i], g["s"][0, i]) for i in range(PROBE_SGS)]
        return self.sgs

    def eval(self, dir):
        if self.sgs is None:
            raise ValueError("LightProbe.eval before gather_light")
        return probe_eval(self._rec, _f3(dir)[None, :])[0, 0]


def render(tree, cam, film, **kw):
    return tree.render(cam, film, **kw)


def tiles_per_rank(film, nranks):
    return lib().vrt_tiles_per_rank(C.byref(film.c), int(nranks))


def tile_deal_map(film, nranks):
    """The library's tile deal as (nty, ntx) arrays: each tile's rank and its
    index in that rank's packed buffer (vrt_tile_deal_map)."""
    ntx, nty = film.nx // 8, film.ny // 8
    rk = np.zeros((nty, ntx), np.int32)
    sl = np.zeros((nty, ntx), np.int32)
    check(lib().vrt_tile_deal_map(C.byref(film.c), int(nranks), ptr(rk, _ffi.i32p), ptr(sl, _ffi.i32p)),
          "vrt_tile_deal_map")
    return rk, sl


def unpack_tiles_device(film, nranks, d_gathered_ptr, d_image_ptr, stream_ptr=None):
    check(lib().vrt_unpack_tiles_device(C.byref(film.c), int(nranks), C.c_void_p(d_gathered_ptr),
                                        C.c_void_p(d_image_ptr),
                                        C.c_void_p(stream_ptr) if stream_ptr else None),
          "vrt_unpack_tiles_device")


def pack_tiles_c_device(film, rank, nranks, comps, d_image_ptr, d_packed_ptr, stream_ptr=None):
    """Rank `rank`'s tiles of a (ny, nx, comps) device image -> its packed
    buffer (vrt_pack_tiles_c_device; config 5: comps = 1)."""
    check(lib().vrt_pack_tiles_c_device(C.byref(film.c), int(rank), int(nranks), int(comps), C.c_void_p(d_image_ptr),
                                        C.c_void_p(d_packed_ptr), C.c_void_p(stream_ptr) if stream_ptr else None),
          "vrt_pack_tiles_c_device")


def unpack_tiles_c_device(film, nranks, comps, d_gathered_ptr, d_image_ptr, stream_ptr=None):
    """Rank 0 after the gather: nranks packed buffers -> the (ny, nx, comps)
    image (vrt_unpack_tiles_c_device)."""
    check(lib().vrt_unpack_tiles_c_device(C.byref(film.c), int(nranks), int(comps), C.c_void_p(d_gathered_ptr),
                                          C.c_void_p(d_image_ptr), C.c_void_p(stream_ptr) if stream_ptr else None),
          "vrt_unpack_tiles_c_device")


def intersect_triangle3(orig, direction, v0, v1, v2):
    """VRT/raytri.h:5-7 -> (ret, t, u, v); t/u/v only meaningful when ret == 1."""
    a = [np.ascontiguousarray(np.asarray(x, np.float64).reshape(3)) for x in (orig, direction, v0, v1, v2)]
    t, u, v = C.c_double(), C.c_double(), C.c_double()
    r = lib().intersect_triangle3(*[ptr(x, _ffi.f64p) for x in a], C.byref(t), C.byref(u), C.byref(v))
    return r, t.value, u.value, v.value


def tri_box_overlap(center, half, tri):
    """VRT/tribox2.h:6 -> 1/0."""
    c = np.ascontiguousarray(np.asarray(center, np.float32).reshape(3))
    h = np.ascontiguousarray(np.asarray(half, np.float32).reshape(3))
    t = np.ascontiguousarray(np.asarray(tri, np.float32).reshape(9))
    return lib().triBoxOverlap(ptr(c, _ffi.f32p), ptr(h, _ffi.f32p), ptr(t, _ffi.f32p))


def hdr_bytes(img):
    """The exact bytes stbi_write_hdr would write for img (h, w, comp)."""
    img = np.ascontiguousarray(np.asarray(img, np.float32))
    h, w = img.shape[:2]
    comp = 1 if img.ndim == 2 else img.shape[2]
    n = lib().vrt_write_hdr_mem(w, h, comp, ptr(img, _ffi.f32p), None, 0)
    if n == 0:
        raise VrtError(_ffi.VRT_E_INVALID, "vrt_write_hdr_mem")
    buf = np.zeros(-n, np.uint8)
    n2 = lib().vrt_write_hdr_mem(w, h, comp, ptr(img, _ffi.f32p), ptr(buf, _ffi.u8p), -n)
    assert n2 == -n
    return buf.tobytes()


def hdr_bytes_from_rgbe(rgbe):
    """stbi_write_hdr bytes from packed RGBE (h, w, 4) uint8 (vrt_write_hdr_rgbe_mem)."""
    rgbe = np.ascontiguousarray(np.asarray(rgbe, np.uint8))
    h, w = rgbe.shape[:2]
    n = lib().vrt_write_hdr_rgbe_mem(w, h, ptr(rgbe, _ffi.u8p), None, 0)
    if n == 0:
        raise VrtError(_ffi.VRT_E_INVALID, "vrt_write_hdr_rgbe_mem")
    buf = np.zeros(-n, np.uint8)
    assert lib().vrt_write_hdr_rgbe_mem(w, h, ptr(rgbe, _ffi.u8p), ptr(buf, _ffi.u8p), -n) == -n
    return buf.tobytes()


def rgbe_device(d_img_ptr, w, h, comp, d_rgbe_ptr, stream_ptr=None):
    """k_rgbe: pack a device float image (w*h*comp) into w*h*4 RGBE bytes."""
    check(lib().vrt_rgbe_device(C.c_void_p(d_img_ptr), int(w), int(h), int(comp), C.c_void_p(d_rgbe_ptr),
                                None if stream_ptr is None else C.c_void_p(stream_ptr)), "vrt_rgbe_device")


def write_hdr_device(path, d_img_ptr, w, h, comp=3, stream_ptr=None):
    """stbi_write_hdr of a device-resident image: RGBE packed on the GPU,
    4 bytes/pixel copied back, RLE on the host.  Byte-identical to write_hdr."""
    import torch
    rgbe = torch.empty(int(w) * int(h) * 4, dtype=torch.uint8, device="cuda")
    rgbe_device(d_img_ptr, w, h, comp, rgbe.data_ptr(), stream_ptr)
    torch.cuda.synchronize()
    host = rgbe.cpu().numpy()
    return lib().vrt_write_hdr_rgbe(str(path).encode(), int(w), int(h), ptr(host, _ffi.u8p)) == 1


def write_hdr(path, img):
    """stbi_write_hdr(path, w, h, comp, data): True on success."""
    img = np.ascontiguousarray(np.asarray(img, np.float32))
    h, w = img.shape[:2]
    comp = 1 if img.ndim == 2 else img.shape[2]
    return lib().vrt_write_hdr(str(path).encode(), w, h, comp, ptr(img, _ffi.f32p)) == 1


def sweep_pose(root_min, root_max, i, n):
    """Camera-sweep pose i of n -> (fov, eye, spot, up)."""
    mn, mx = _f3(root_min), _f3(root_max)
    eye, spot, up = np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
    fov = C.c_float()
    check(lib().vrt_sweep_pose(ptr(mn, _ffi.f32p), ptr(mx, _ffi.f32p), int(i), int(n), ptr(eye, _ffi.f32p),
                               ptr(spot, _ffi.f32p), ptr(up, _ffi.f32p), C.byref(fov)), "vrt_sweep_pose")
    return fov.value, eye, spot, up


def device_selftest_order(dist, hit_mask, depth=None, lengths=None, device=0):
    """The kernels' travorder sort and min_element code on arbitrary inputs
    (vrt_device_selftest_order): dist (n, 8) f32, hit_mask (n,) -> (n, 6)
    u32 order words; depth (m, k) f32 + lengths (m,) -> (m,) first argmin."""
    dist = np.ascontiguousarray(np.asarray(dist, np.float32).reshape(-1, 8))
    hm = np.ascontiguousarray(np.asarray(hit_mask, np.uint32).reshape(-1))
    n = dist.shape[0]
    assert hm.shape[0] == n
    orders = np.zeros((n, 6), np.uint32)
    m, stride, dep, ln, am = 0, 0, None, None, None
    if depth is not None:
        dep = np.ascontiguousarray(np.asarray(depth, np.float32))
        m, stride = dep.shape
        ln = np.ascontiguousarray(np.asarray(lengths, np.int32).reshape(-1))
        assert ln.shape[0] == m
        am = np.zeros(m, np.int32)
    check(lib().vrt_device_selftest_order(device, ptr(dist, _ffi.f32p), ptr(hm, _ffi.u32p), n,
                                          ptr(orders, _ffi.u32p), ptr(dep, _ffi.f32p), ptr(ln, _ffi.i32p), m,
                                          stride, ptr(am, _ffi.i32p)), "vrt_device_selftest_order")
    return orders, am


def device_selftest_chain(cases, device=0):
    """The walk's chain-order code on arbitrary expansions
    (vrt_device_selftest_chain): cases (n, 21) f32 = node box min, max, ray
    origin, direction, root box min, max, ord_wmin -> (n, 6) u32 {hit mask,
    sorted order | count << 24, chain order | count << 24, general-form chain
    order | count << 24, flags, the walk's own expansion | count << 24}."""
    cases = np.ascontiguousarray(np.asarray(cases, np.float32).reshape(-1, 21))
    n = cases.shape[0]
    out = np.zeros((n, 6), np.uint32)
    check(lib().vrt_device_selftest_chain(device, ptr(cases, _ffi.f32p), n, ptr(out, _ffi.u32p)),
          "vrt_device_selftest_chain")
    return out


DIGEST_ITEMS = 10  # include/vrt.h VRT_DIGEST_ITEMS


def digest(data, device=None, misalign=0):
    """The digest of include/vrt.h over `data`'s bytes (a whole number of
    32-bit words): the host statement (device None, vrt_digest_host) or the
    kernel's own code on `device`, from a 16-byte-aligned buffer + misalign
    (vrt_device_selftest_digest)."""
    a = np.ascontiguousarray(data)
    b = a.view(np.uint8).reshape(-1) if a.size else np.zeros(0, np.uint8)
    out = C.c_uint64()
    p = b.ctypes.data_as(C.c_void_p) if b.size else None
    if device is None:
        check(lib().vrt_digest_host(p, b.size, C.byref(out)), "vrt_digest_host")
    else:
        check(lib().vrt_device_selftest_digest(int(device), p, b.size, int(misalign), C.byref(out)),
              "vrt_device_selftest_digest")
    return out.value


def build_id():
    """Source hash libvrt.so was built from (tools/build_id.py)."""
    return lib().vrt_build_id().decode()


def build_flag(name):
    """A path-selecting compile-time switch of libvrt.so's kernel build
    (vrt_build_flag), e.g. "VRT_SEC_SPILL_T" (config 5's compaction
    threshold; 0 = no compaction)."""
    v = C.c_int64()
    check(lib().vrt_build_flag(name.encode(), C.byref(v)), "vrt_build_flag")
    return v.value


TEST_FORCE_DEFER = 1  # include/vrt.h VRT_TEST_FORCE_DEFER
TEST_FAIL_LAUNCH = 2  # include/vrt.h VRT_TEST_FAIL_LAUNCH
TEST_SPILL_ALL = 4  # include/vrt.h VRT_TEST_SPILL_ALL
TEST_VIRTUAL_RANKS = 8  # include/vrt.h VRT_TEST_VIRTUAL_RANKS (count << 8)
TEST_STREAM_LEFTOVER = 16  # include/vrt.h VRT_TEST_STREAM_LEFTOVER
TEST_LIGHT_TAIL = 32  # include/vrt.h VRT_TEST_LIGHT_TAIL
TEST_PRIM_TAIL = 64  # include/vrt.h VRT_TEST_PRIM_TAIL
TEST_SEC_DEFER = 128  # include/vrt.h VRT_TEST_SEC_DEFER
TEST_SMALL_BATCH_CHUNK = 0x10000  # include/vrt.h VRT_TEST_SMALL_BATCH_CHUNK
TEST_SMALL_PROBE_CHUNK = 0x20000  # include/vrt.h VRT_TEST_SMALL_PROBE_CHUNK
TEST_SMALL_BEAM_ENTRY = 0x40000  # include/vrt.h VRT_TEST_SMALL_BEAM_ENTRY
TEST_UPDATE_TOO_LARGE = 0x80000  # include/vrt.h VRT_TEST_UPDATE_TOO_LARGE
TEST_MULTI_REFUSE_LAST = 0x100000  # include/vrt.h VRT_TEST_MULTI_REFUSE_LAST
TEST_MULTI_DIVERGE = 0x200000  # include/vrt.h VRT_TEST_MULTI_DIVERGE


def set_test_flags(flags):
    """Test hook (vrt_set_test_flags): flags read by every later launch."""
    check(lib().vrt_set_test_flags(int(flags)), "vrt_set_test_flags")


def test_flags():
    """The current vrt_set_test_flags value (vrt_test_flags)."""
    return int(lib().vrt_test_flags())


def device_count():
    n = C.c_int32()
    check(lib().vrt_device_count(C.byref(n)), "vrt_device_count")
    return n.value


def device_selftest(mt_in=None, sat_in=None, device=0):
    """Run the kernels' own MT / SAT code on the device over n cases."""
    n = len(mt_in) if mt_in is not None else len(sat_in)
    mt_out = np.zeros((n, 4), np.float64) if mt_in is not None else None
    sat_out = np.zeros(n, np.int32) if sat_in is not None else None
    mi = None if mt_in is None else np.ascontiguousarray(np.asarray(mt_in, np.float64).reshape(n, 15))
    si = None if sat_in is None else np.ascontiguousarray(np.asarray(sat_in, np.float32).reshape(n, 15))
    check(lib().vrt_device_selftest(int(device), ptr(mi, _ffi.f64p), ptr(mt_out, _ffi.f64p),
                                    ptr(si, _ffi.f32p), ptr(sat_out, _ffi.i32p), n), "vrt_device_selftest")
    return mt_out, sat_out
