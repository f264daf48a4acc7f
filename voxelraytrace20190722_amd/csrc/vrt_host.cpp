// vrt_host.cpp -- host side of libvrt.so: the C ABI of include/vrt.h.
//
//  * octree build (gi::ray_march_init, VRT/voxel_octree.cc:27-75) as a
//    parallel per-triangle descent + sort, flattened to the BFS child-block
//    layout the kernels read (DESIGN.md "Data layout in HBM");
//  * scene upload, render / ray-march orchestration on a HIP stream;
//  * camera (VRT/camera.cc:65-112) and the legacy intersect_triangle3 /
//    triBoxOverlap symbols, all through vrt_math.h (the kernels' own code).
//
// VRT/x = /root/reference/VoxelRayTrace20190722/x
#include "../../include/vrt.h"
#include "vrt_error.h"
#include "vrt_internal.h"
#include "vrt_sg.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <limits>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace vrt;

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static thread_local std::string g_err;

static int vfail(int code, const char *fmt, va_list ap)
{
        char buf[512];
        vsnprintf(buf, sizeof buf, fmt, ap);
        g_err = buf;
        return code;
}

static int fail(int code, const char *fmt, ...)
{
        va_list ap;
        va_start(ap, fmt);
        vfail(code, fmt, ap);
        va_end(ap);
        return code;
}

// shared with the ingest sources (vrt_obj.cpp, vrt_tga.cpp); hidden symbol
int vrt::set_error(int code, const char *fmt, ...)
{
        va_list ap;
        va_start(ap, fmt);
        vfail(code, fmt, ap);
        va_end(ap);
        return code;
}

#define HIPCHK(expr)                                                             \
        do {                                                                     \
                hipError_t e_ = (expr);                                          \
                if (e_ != hipSuccess)                                            \
                        return fail(VRT_E_DEVICE, "%s failed: %s", #expr,       \
                                    hipGetErrorString(e_));                      \
        } while (0)

extern "C" const char *vrt_last_error(void) { return g_err.c_str(); }

extern "C" const char *vrt_status_string(int s)
{
        switch (s) {
        case VRT_OK: return "ok";
        case VRT_E_INVALID: return "invalid argument";
        case VRT_E_NOMEM: return "out of host memory";
        case VRT_E_DEVICE: return "HIP runtime error";
        case VRT_E_NODEVICE: return "no usable gfx950 device";
        case VRT_E_IO: return "i/o error";
        default: return "unknown status";
        }
}

static double now_ms()
{
        using namespace std::chrono;
        return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// ---------------------------------------------------------------------------
// legacy reference symbols
// ---------------------------------------------------------------------------
extern "C" int intersect_triangle3(double orig[3], double dir[3],
                                   double vert0[3], double vert1[3],
                                   double vert2[3], double *t, double *u,
                                   double *v)
{
        return mt_isect(orig, dir, vert0, vert1, vert2, t, u, v);
}

extern "C" int triBoxOverlap(float boxcenter[3], float boxhalfsize[3],
                             float triverts[3][3])
{
        return tri_box_overlap(boxcenter, boxhalfsize, &triverts[0][0]);
}

// ---------------------------------------------------------------------------
// camera (VRT/camera.cc:65-112)
// ---------------------------------------------------------------------------
extern "C" int vrt_camera_init(float fov, const float eye[3],
                               const float spot[3], const float up[3],
                               float near_, float far_, vrt_camera *out)
{
        if (!eye || !spot || !up || !out)
                return fail(VRT_E_INVALID, "vrt_camera_init: null argument");
        const f3 e = mk3(eye[0], eye[1], eye[2]);
        const f3 fwd = normalize(mk3(spot[0], spot[1], spot[2]) - e);
        const f3 s = normalize(cross(fwd, mk3(up[0], up[1], up[2])));
        const f3 u = normalize(cross(s, fwd));
        const f3 nf = -fwd;
        const float C[16] = { s.x, s.y, s.z, 0.f, u.x, u.y, u.z, 0.f,
                              nf.x, nf.y, nf.z, 0.f, e.x, e.y, e.z, 1.f };
        std::memcpy(out->C, C, sizeof C);
        out->fov = fov;
        out->near_ = near_;
        out->far_ = far_;
        // point_transform(C_, {}): dot(C, (0,0,0,1)) then /= w
        // (VRT/graphics_math.h:1063-1070)
        float r[4];
        for (int k = 0; k < 4; ++k) {
                float acc = 0.0f;
                acc += C[k] * 0.0f;
                acc += C[4 + k] * 0.0f;
                acc += C[8 + k] * 0.0f;
                acc += C[12 + k] * 1.0f;
                r[k] = acc;
        }
        const float w = r[3];
        for (int k = 0; k < 3; ++k)
                out->origin[k] = r[k] / w;
        return VRT_OK;
}

static float cam_zplane(const vrt_camera *cam, const vrt_film *film)
{
        // -(film.h / (2 * std::tanf(fov / 2)))  (VRT/camera.cc:100)
        return -(film->h / (2.0f * tanf(cam->fov / 2.0f)));
}

static void fill_cam_params(const vrt_camera *cam, const vrt_film *film,
                            CamParams *cp)
{
        for (int k = 0; k < 3; ++k) {
                cp->s[k] = cam->C[k];
                cp->u[k] = cam->C[4 + k];
                cp->nf[k] = cam->C[8 + k];
                cp->e[k] = cam->C[12 + k];
                cp->origin[k] = cam->origin[k];
        }
        cp->z = cam_zplane(cam, film);
        cp->tmin = cam->near_;
        cp->tmax = cam->far_;
        cp->nx = film->nx;
        cp->ny = film->ny;
}

static int gen_rays(const vrt_camera *cam, const vrt_film *film, int px,
                    int py, vrt_ray *out, int n)
{
        if (!cam || !film || !out)
                return fail(VRT_E_INVALID, "gen_rays: null argument");
        if (px < 0 || px >= film->nx || py < 0 || py >= film->ny)
                return fail(VRT_E_INVALID, "gen_rays: pixel (%d,%d) outside film", px, py);
        CamParams cp;
        fill_cam_params(cam, film, &cp);
        for (int s = 0; s < n; ++s) {
                const float sx = n == 4 ? sample_x(s) : 0.5f;
                const float sy = n == 4 ? sample_y(s) : 0.5f;
                const f3 d = camera_dir(cp.s, cp.u, cp.nf, cp.e, cp.z, cp.nx, cp.ny,
                                        px, py, sx, sy);
                for (int k = 0; k < 3; ++k)
                        out[s].o[k] = cp.origin[k];
                out[s].d[0] = d.x;
                out[s].d[1] = d.y;
                out[s].d[2] = d.z;
                out[s].tmin = cp.tmin;
                out[s].tmax = cp.tmax;
        }
        return VRT_OK;
}

extern "C" int vrt_camera_defer_bound(const vrt_camera *cam, const vrt_film *film, int64_t *bound)
{
        if (!cam || !film || !bound || film->nx < 1 || film->ny < 1)
                return fail(VRT_E_INVALID, "vrt_camera_defer_bound: bad argument");
        CamParams cp;
        fill_cam_params(cam, film, &cp);
        *bound = camera_defer_bound(cp);
        return VRT_OK;
}

extern "C" int vrt_gen_rays4(const vrt_camera *cam, const vrt_film *film,
                             int px, int py, vrt_ray out[4])
{
        return gen_rays(cam, film, px, py, out, 4);
}

extern "C" int vrt_gen_rays1(const vrt_camera *cam, const vrt_film *film,
                             int px, int py, vrt_ray out[1])
{
        return gen_rays(cam, film, px, py, out, 1);
}

extern "C" int vrt_make_ray(const float o[3], const float d[3], float tmin,
                            float tmax, vrt_ray *out)
{
        if (!o || !d || !out)
                return fail(VRT_E_INVALID, "vrt_make_ray: null argument");
        const f3 dn = normalize(mk3(d[0], d[1], d[2]));
        for (int k = 0; k < 3; ++k)
                out->o[k] = o[k];
        out->d[0] = dn.x;
        out->d[1] = dn.y;
        out->d[2] = dn.z;
        out->tmin = tmin;
        out->tmax = tmax;
        return VRT_OK;
}

extern "C" int vrt_aabb_isect(const float box[6], const vrt_ray *ray)
{
        if (!box || !ray)
                return 0;
        const f3 o = mk3(ray->o[0], ray->o[1], ray->o[2]);
        const f3 di = mk3(dinv_of(ray->d[0]), dinv_of(ray->d[1]), dinv_of(ray->d[2]));
        return aabb_isect(box, box + 3, o, di, ray->tmin, ray->tmax) ? 1 : 0;
}

// ---------------------------------------------------------------------------
// octree build
// ---------------------------------------------------------------------------
namespace {

struct Box {
        float mn[3], mx[3];
};

// split() child box (VRT/voxel_octree.cc:30-35)
inline Box child_box(const Box &p, int i)
{
        Box c;
        const int m[3] = { (i & 4) ? 1 : 0, (i & 2) ? 1 : 0, (i & 1) ? 1 : 0 };
        for (int k = 0; k < 3; ++k) {
                const float half = (p.mx[k] - p.mn[k]) / 2.0f;
                c.mn[k] = p.mn[k] + (float)m[k] * half;
                c.mx[k] = c.mn[k] + half;
        }
        return c;
}

// Triangle::is_overlap (VRT/voxel_octree.cc:486-492)
inline bool overlaps(const float *tri9, const Box &b)
{
        float c[3], h[3];
        for (int k = 0; k < 3; ++k) {
                c[k] = (b.mn[k] + b.mx[k]) * .5f;
                h[k] = (b.mx[k] - b.mn[k]) / 2.f;
        }
        return tri_box_overlap(c, h, tri9) == 1;
}

struct BuildOut {
        // internal node keys per depth (path code, 3 bits per level)
        std::vector<std::vector<uint32_t>> internal;
        // (leaf code << 32 | tri) at max depth
        std::vector<uint64_t> refs;
};

// Descend one triangle: the set of nodes insert() reaches for it.  A node is
// split iff some triangle overlaps it (and all its ancestors) above
// max_depth; a max-depth leaf lists exactly those triangles.
void descend(const float *tri9, uint32_t tri, const Box &b, int depth,
             int max_depth, uint32_t code, BuildOut &o);

// The same for a light probe (LightProbe::is_overlap, VRT/voxel_octree.cc:
// 567-586): insert() splits and descends for any voxel alike.
void descend_probe(const vrt_probe &pb, uint32_t k, const Box &b, int depth, int max_depth, uint32_t code,
                   BuildOut &o)
{
        if (!probe_overlap(mk3(pb.o[0], pb.o[1], pb.o[2]), pb.r, b.mn, b.mx))
                return;
        if (depth == max_depth) {
                o.refs.push_back(((uint64_t)code << 32) | k);
                return;
        }
        o.internal[depth].push_back(code);
        for (int i = 0; i < 8; ++i)
                descend_probe(pb, k, child_box(b, i), depth + 1, max_depth, (code << 3) | (uint32_t)i, o);
}

void descend(const float *tri9, uint32_t tri, const Box &b, int depth,
             int max_depth, uint32_t code, BuildOut &o)
{
        if (!overlaps(tri9, b))
                return;
        if (depth == max_depth) {
                o.refs.push_back(((uint64_t)code << 32) | tri);
                return;
        }
        o.internal[depth].push_back(code);
        for (int i = 0; i < 8; ++i)
                descend(tri9, tri, child_box(b, i), depth + 1, max_depth,
                        (code << 3) | (uint32_t)i, o);
}

uint32_t vox_of(uint32_t code, int depth)
{
        uint32_t ix = 0, iy = 0, iz = 0;
        for (int l = depth - 2; l >= 0; --l) {
                const uint32_t ci = (code >> (3 * l)) & 7u;
                ix = (ix << 1) | ((ci >> 2) & 1u);
                iy = (iy << 1) | ((ci >> 1) & 1u);
                iz = (iz << 1) | (ci & 1u);
        }
        return ix | (iy << 10) | (iz << 20);
}

}  // namespace

// Bands of vrt_render's host-output path: tile-row bands rendered
// alternately on two streams (each a half-chip persistent grid, as with
// frames in flight), each band's D2H copy queued as soon as it is rendered,
// so the copies of the first bands run beside the renders of the last.
constexpr int kOutBands = 4;
struct HostOut {
        Staging img;  // nx*ny*3 floats (pixels outside the tile grid stay 0) and their pinned copy; on cp
        int nx = 0, ny = 0;
        Stream st2, cp;
        Event ev_r[kOutBands], ev_c[kOutBands];
        Event ev_j;  // second render stream joined back
};

// One set of the full trace's scene scratch (vrt_scene::ts).
struct TraceSet {
        DevMem lm;   // nodes x (LMRec + float4 cone record) + the finiteness flag
        DevMem rec;  // split-trace records (64 B per sample), the cone step table
        float steps_key[2] = { -1.f, -1.f };  // (mindist, maxdist) the step table holds
        LastUse use;
};

// The side stream of a compaction set's deferred-pixel walk and its fork /
// join events (SideLaunch is the view launch_secondary takes): all three or
// none.
struct SideStream {
        Stream st;
        Event fork, join;
};

struct vrt_scene {
        int device = 0;
        int max_depth = 0;
        int ntri = 0;
        std::vector<NodeRec> nodes;
        std::vector<uint32_t> node_vox;
        std::vector<RefRec48> refs48;   // one of the two leaf-record formats
        std::vector<RefRec64> refs64;   // (wide_leaves: RefRec64)
        bool wide_leaves = false;
        std::vector<uint32_t> ref_tri;  // triangle id per leaf-list entry
        std::vector<TriPos> tri_pos;
        std::vector<TriAttr> tri_attr;
        std::vector<MatRec> mats;
        std::vector<TexRec> texs;
        int64_t tex_bytes = 0;
        vrt_scene_info_t info{};
        std::vector<int64_t> level_begin;  // BFS level l (1-based) = [lb[l-1], lb[l])
        // light probes as voxels (vrt_scene_create_probes; empty otherwise):
        // the probes, per node its probe list or child mask (ProbeDev::pnode),
        // the concatenated leaf lists, the stored SGs (14 per probe), and their
        // device copies: the probes and the SGs, whose sizes never change, in
        // d_probe; pnode (one per node) and pref (one per probe reference)
        // follow the geometry and have an owner each, with its capacity, as
        // g_nodes ... g_xnodes have (vrt_scene_update_probes)
        std::vector<vrt_probe> probes;
        std::vector<uint2> pnode;
        std::vector<uint32_t> pref;
        std::vector<vrt_sg> probe_sgs;
        int64_t probe_leaves = 0;
        DevMem d_probe, g_pnode, g_pref;
        ProbeDev pdev{};
        // the stored SGs' device copy (in d_probe), read by the kernels that
        // shade a probe hit.  The host copy probe_sgs is what the host
        // shaders read; sgs_stale: a device gather (vrt_trace_frame_probes_
        // device) wrote the device copy last and the host copy is fetched
        // before its next reader (sync_probe_sgs)
        float *d_sgs = nullptr;
        bool sgs_stale = false;
        Event sg_ev;  // vrt_trace_frame_probes_device: the gather is done
        // full trace: two sets of {light-map block (LMRec + cone-descent
        // records + finiteness flag), split-trace records}, taken by
        // alternate light-map builds so that one frame's cone-traced shading
        // runs beside the next frame's light pass; each with the event of its
        // last user.  lm_cur = the set with the latest light map (-1: none).
        // The light pass's own scratch (keys, sort) is used on the scene
        // stream only.
        TraceSet ts[2];
        int ts_next = 0;
        int lm_cur = -1;
        int64_t lm_stats[3] = {};  // the last build's samples, hits, tail samples (vrt_lightmap_stats)
        DevMem d_light;
        // config-5 ray compaction (SpillQueues): round counters + two record
        // queues of spill_cap chunks each; two sets, used by alternate
        // frames (two config-5 frames in flight on two streams), each with
        // the event of its last launch
        DevMem d_spill[2];
        uint32_t spill_cap[2] = {};  // chunks per queue
        int64_t spill_px[2] = {};    // deferred-pixel list capacity (pixels)
        LastUse spill_use[2];
        hipStream_t spill_stream[2] = {};  // the set's last user (a stream keeps its set)
        SideStream spill_side[2];
        // multi-rank tile deals tabled on the device (RenderParams::tile_xy),
        // one per (tiles, ranks, rank) used, built on first use by a kernel
        // on that call's stream (ev), kept until the scene is destroyed
        struct DealMap {
                int ntx, nty, nranks, rank;
                DevMem d;
                LastUse built;
        };
        std::vector<DealMap> dmaps;
        PinnedMem h_spill;                 // per set, its last launch's round counters (ctr[0..7])
        uint32_t spill_want = 0;           // queue-0 chunks the next launch sizes for (0: first estimate)
        int spill_next = 0;
        int spill_last = -1;  // the set the last config-5 launch compacted with (vrt_secondary_spill_counts)
        // device: d_mem holds what no update touches or resizes (TriPos,
        // TriAttr, materials, textures, the work queues); the arrays whose size
        // follows the geometry have an owner each, with its capacity, so that
        // vrt_scene_update reallocates only the ones that must grow
        DevMem d_mem;
        DevMem g_nodes, g_vox, g_refs, g_xnodes;  // g_refs: [pad | per-record boxes | records]
        bool rboxes = false;  // the per-record boxes are there (has_ref_boxes at the last build)
        DevScene dev{};
        // vrt_scene_update: the build's scratch (kept between updates, not part
        // of vrt_scene_scratch_bytes), the caller's stream joined in, the
        // events of the GPU part and the last update's {total, GPU, copy back,
        // host} ms; owned: a rank scene of a vrt_multi handle (no update)
        BuildScratch bscratch;
        // the host mirrors' other halves: an update fills these and swaps, so a
        // steady animation neither allocates nor frees (nor zero-fills) them
        std::vector<NodeRec> up_nodes;
        std::vector<uint32_t> up_vox, up_ref_tri;
        std::vector<uint2> up_pnode;  // ... and a probe scene's (vrt_scene_update_probes)
        std::vector<uint32_t> up_pref;
        std::vector<vrt_probe> up_probes;
        Event up_in, up_e0, up_e1;
        GrowMem digest;  // vrt_scene_digest: the ten words (80 B), made on first use
        double up_ms[4] = {};
        bool updated = false;
        bool owned = false;
        // chain order: per axis the smallest spacing of the
        // two child centres over the internal nodes, 0 = off (chain_spacing)
        float ord_wmin[3] = {};
        Stream stream;
        Event ev0, ev1;
        bool timed = false;
        // persistent-render work queues (WorkQueue, vrt_internal.h): a ring
        // of kQueueSlots counter sets, each with its bases and the event of
        // its last launch
        uint32_t *d_queue = nullptr;
        uint32_t q_base[kQueueSlots][8] = {};
        LastUse q_use[kQueueSlots];
        int q_next = 0;
        // beam-entry records (VRT_BEAM_ENTRY, vrt_internal.h): one buffer per
        // ring slot, grown to the largest share rendered on it and protected
        // by the slot's q_use like its counters; entry_slot / entry_units:
        // the last persistent fast-only launch's (vrt_debug_beam_entries)
        DevMem d_entry[kQueueSlots];
        int entry_slot = -1;
        int64_t entry_units = 0;
        Event lm_ev;  // vrt_trace_frame_device: the light map is filtered
        // vrt_render's host-output path (render_to_host): a device image kept
        // between calls, its pinned host staging copy, a second render stream
        // and a copy stream, and an event per band
        HostOut ho;
        // vrt_ray_march_batch: device ray / hit buffers and pinned staging
        // kept between calls (grown as needed)
        Staging rays, hits;
        // vrt_trace_batch / vrt_cone_trace_batch (host arrays): one chunk's
        // inputs and outputs on the device and their pinned staging, kept
        // between calls (grown as needed, never beyond one chunk)
        Staging tb;
        // every entry point that launches work on the scene holds mu (one
        // host thread at a time; device work on several streams is ordered
        // by the events above)
        std::mutex mu;
};

static int finish_tree(vrt_scene *s, const vrt_scene_desc *d, const Box &root, const std::vector<uint64_t> &refs,
                       int64_t ninternal);
static int check_device(int device);

static int build_tree(vrt_scene *s, const vrt_scene_desc *d, bool on_device)
{
        const int D = s->max_depth;
        const int n = d->ntri;
        // root = AABB{} merged with every triangle AABB, in input order
        // (VRT/voxel_octree.cc:70-72; AABB(Iter,Iter) graphics_math.h:1240-1251)
        Box root;
        for (int k = 0; k < 3; ++k) {
                root.mn[k] = kFltMax;
                root.mx[k] = -kFltMax;
        }
        for (int i = 0; i < n; ++i) {
                const float *p = d->pos + 9 * (size_t)i;
                float tmn[3] = { kFltMax, kFltMax, kFltMax };
                float tmx[3] = { -kFltMax, -kFltMax, -kFltMax };
                for (int v = 0; v < 3; ++v)
                        for (int k = 0; k < 3; ++k) {
                                tmn[k] = std_min(tmn[k], p[3 * v + k]);
                                tmx[k] = std_max(tmx[k], p[3 * v + k]);
                        }
                for (int k = 0; k < 3; ++k) {
                        root.mn[k] = std_min(root.mn[k], tmn[k]);
                        root.mx[k] = std_max(root.mx[k], tmx[k]);
                }
        }
        // then every probe's get_aabb() = AABB3D{o_ - r_, o_ + r_}, in probe
        // order (VRT/voxel_octree.cc:541-544; main.cc pushes the probes
        // behind the triangles)
        for (const vrt_probe &pb : s->probes)
                for (int k = 0; k < 3; ++k) {
                        root.mn[k] = std_min(root.mn[k], pb.o[k] - pb.r);
                        root.mx[k] = std_max(root.mx[k], pb.o[k] + pb.r);
                }

        if (on_device) {
                // level-synchronous descent, sorts, flatten and masks on the GPU
                DeviceBuild db;
                std::string err;
                int rc = check_device(s->device);
                if (rc)
                        return rc;
                if (build_tree_device(s->device, d->pos, n, root.mn, root.mx, D, s->probes.data(),
                                      (int)s->probes.size(), &db, &err) != hipSuccess) {
                        if (db.too_large)
                                return fail(VRT_E_INVALID, "%s", err.c_str());
                        return fail(VRT_E_DEVICE, "device octree build: %s", err.c_str());
                }
                s->nodes.swap(db.nodes);
                s->node_vox.swap(db.node_vox);
                s->level_begin.swap(db.level_begin);
                s->pnode.swap(db.pnode);
                s->pref.swap(db.pref);
                s->probe_leaves = db.probe_leaves;
                s->info.build_device_ms = db.device_ms;
                return finish_tree(s, d, root, db.refs, db.ninternal);
        }
        // parallel per-triangle descent
        unsigned nth = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
        if (n < 4096)
                nth = 1;
        std::vector<BuildOut> outs(nth);
        for (auto &o : outs)
                o.internal.resize(D + 1);
        {
                std::atomic<int> next{ 0 };
                auto work = [&](unsigned t) {
                        BuildOut &o = outs[t];
                        for (;;) {
                                const int i0 = next.fetch_add(1024);
                                if (i0 >= n)
                                        break;
                                const int i1 = std::min(n, i0 + 1024);
                                for (int i = i0; i < i1; ++i)
                                        descend(d->pos + 9 * (size_t)i, (uint32_t)i, root, 1, D, 0u, o);
                        }
                };
                std::vector<std::thread> th;
                for (unsigned t = 1; t < nth; ++t)
                        th.emplace_back(work, t);
                work(0);
                for (auto &x : th)
                        x.join();
        }
        // the probes, after all triangles and in probe order: they split
        // the nodes they overlap like any voxel; their leaf entries stay apart
        // from the triangles' (prefs), so that a leaf's a / b words and the
        // content masks keep counting triangles only
        BuildOut pout;
        pout.internal.resize(D + 1);
        for (size_t k = 0; k < s->probes.size(); ++k)
                descend_probe(s->probes[k], (uint32_t)k, root, 1, D, 0u, pout);
        std::vector<uint64_t> prefs;
        prefs.swap(pout.refs);
        std::sort(prefs.begin(), prefs.end());  // (leaf code, probe index)
        // merge
        std::vector<std::vector<uint32_t>> internal(D + 1);
        for (int l = 1; l < D; ++l) {
                size_t tot = pout.internal[l].size();
                for (auto &o : outs)
                        tot += o.internal[l].size();
                internal[l].reserve(tot);
                internal[l].insert(internal[l].end(), pout.internal[l].begin(), pout.internal[l].end());
                for (auto &o : outs) {
                        internal[l].insert(internal[l].end(), o.internal[l].begin(), o.internal[l].end());
                        std::vector<uint32_t>().swap(o.internal[l]);
                }
                std::sort(internal[l].begin(), internal[l].end());
                internal[l].erase(std::unique(internal[l].begin(), internal[l].end()), internal[l].end());
        }
        std::vector<uint64_t> refs;
        {
                size_t tot = 0;
                for (auto &o : outs)
                        tot += o.refs.size();
                refs.reserve(tot);
                for (auto &o : outs) {
                        refs.insert(refs.end(), o.refs.begin(), o.refs.end());
                        std::vector<uint64_t>().swap(o.refs);
                }
                // (leaf code, tri index): leaf lists in insertion = input order
                std::sort(refs.begin(), refs.end());
        }

        // flatten: root = node 0; level by level, internal nodes in code
        // order each own the next block of 8 children.
        int64_t ninternal = 0;
        for (int l = 1; l < D; ++l)
                ninternal += (int64_t)internal[l].size();
        const int64_t nnodes = 1 + 8 * ninternal;
        if (nnodes > 0x7FFFFFFF)
                return fail(VRT_E_INVALID, "octree too large (%lld nodes)", (long long)nnodes);
        s->nodes.assign((size_t)nnodes, NodeRec{});
        s->node_vox.assign((size_t)nnodes, 0u);
        std::vector<Box> boxes((size_t)nnodes);
        std::vector<uint32_t> codes((size_t)nnodes);
        std::vector<int32_t> depth_of((size_t)nnodes);
        boxes[0] = root;
        codes[0] = 0;
        depth_of[0] = 1;
        // first node index of each level and the block base of each internal
        // node: internal node j (global order) owns children 1 + 8j ...
        int64_t j_base = 0;  // global index of first internal node at level l
        // level l's nodes occupy a contiguous index range [lv_begin, lv_end)
        int64_t lv_begin = 0, lv_end = 1;
        size_t ref_pos = 0, pref_pos = 0;
        const bool with_probes = !s->probes.empty();
        if (with_probes) {
                s->pnode.assign((size_t)nnodes, make_uint2(0u, 0u));
                s->pref.resize(prefs.size());
                for (size_t i = 0; i < prefs.size(); ++i)
                        s->pref[i] = (uint32_t)(prefs[i] & 0xFFFFFFFFu);
                s->probe_leaves = 0;
        }
        s->level_begin.clear();
        for (int l = 1; l <= D; ++l) {
                s->level_begin.push_back(lv_begin);
                const std::vector<uint32_t> &I = internal[l];  // empty at l == D
                // nodes of this level are in code order (children blocks of
                // the previous level's code-ordered internal nodes)
                size_t ii = 0;
                for (int64_t ni = lv_begin; ni < lv_end; ++ni) {
                        const uint32_t code = codes[ni];
                        NodeRec &nr = s->nodes[ni];
                        for (int k = 0; k < 3; ++k) {
                                nr.bmin[k] = boxes[ni].mn[k];
                                nr.bmax[k] = boxes[ni].mx[k];
                        }
                        s->node_vox[ni] = vox_of(code, l);
                        while (ii < I.size() && I[ii] < code)
                                ++ii;
                        if (l < D && ii < I.size() && I[ii] == code) {
                                const int64_t jg = j_base + (int64_t)ii;
                                const int64_t first = 1 + 8 * jg;
                                nr.a = (uint32_t)first;
                                nr.b = 0;
                                for (int c = 0; c < 8; ++c) {
                                        boxes[first + c] = child_box(boxes[ni], c);
                                        codes[first + c] = (code << 3) | (uint32_t)c;
                                        depth_of[first + c] = l + 1;
                                }
                        } else if (l == D) {
                                // max-depth leaf: its list in refs
                                const uint64_t key = (uint64_t)code << 32;
                                while (ref_pos < refs.size() && refs[ref_pos] < key)
                                        ++ref_pos;
                                const size_t r0 = ref_pos;
                                while (ref_pos < refs.size() && (refs[ref_pos] >> 32) == code)
                                        ++ref_pos;
                                nr.a = kLeafBit | (uint32_t)(ref_pos - r0);
                                nr.b = (uint32_t)r0;
                                if (with_probes) {
                                        while (pref_pos < prefs.size() && prefs[pref_pos] < key)
                                                ++pref_pos;
                                        const size_t p0 = pref_pos;
                                        while (pref_pos < prefs.size() && (prefs[pref_pos] >> 32) == code)
                                                ++pref_pos;
                                        s->pnode[ni] = make_uint2((uint32_t)p0, (uint32_t)(pref_pos - p0));
                                        if (pref_pos > p0)
                                                ++s->probe_leaves;
                                }
                        } else {
                                nr.a = kLeafBit;  // empty leaf above max depth
                                nr.b = 0;
                        }
                }
                // next level: children of this level's internal nodes, in
                // the same (code) order
                const int64_t next_begin = lv_end;
                const int64_t next_end = next_begin + 8 * (int64_t)I.size();
                j_base += (int64_t)I.size();
                lv_begin = next_begin;
                lv_end = next_end;
                if (l < D && lv_begin == lv_end)
                        break;
        }
        s->level_begin.push_back(nnodes);
        // content masks, bottom-up (children always follow their parent):
        // an internal node's b = the children that hold triangles somewhere
        // below.  The kernels never push a child outside this mask: a
        // subtree without triangles cannot hit, so the DFS result is
        // unchanged (the instrumented kernel ignores it to count exactly the
        // reference's visits).
        {
                std::vector<uint8_t> has((size_t)nnodes, 0);
                for (int64_t ni = nnodes - 1; ni >= 0; --ni) {
                        NodeRec &nr = s->nodes[ni];
                        if (nr.a & kLeafBit) {
                                has[ni] = (nr.a & ~kLeafBit) ? 1 : 0;
                        } else {
                                uint32_t m = 0;
                                for (int c = 0; c < 8; ++c)
                                        m |= (uint32_t)has[nr.a + c] << c;
                                nr.b = m;
                                has[ni] = m ? 1 : 0;
                        }
                }
        }
        // the same for the probes, in the side array: an internal node's
        // pnode.x = the children with a probe somewhere below
        if (with_probes) {
                std::vector<uint8_t> has((size_t)nnodes, 0);
                for (int64_t ni = nnodes - 1; ni >= 0; --ni) {
                        const NodeRec &nr = s->nodes[ni];
                        if (nr.a & kLeafBit) {
                                has[ni] = s->pnode[ni].y ? 1 : 0;
                        } else {
                                uint32_t m = 0;
                                for (int c = 0; c < 8; ++c)
                                        m |= (uint32_t)has[nr.a + c] << c;
                                s->pnode[ni] = make_uint2(m, 0u);
                                has[ni] = m ? 1 : 0;
                        }
                }
        }
        return finish_tree(s, d, root, refs, ninternal);
}

// leaf records with inlined vertices + scene info (both build paths)
static int finish_tree(vrt_scene *s, const vrt_scene_desc *d, const Box &root, const std::vector<uint64_t> &refs,
                       int64_t ninternal)
{
        const int64_t nnodes = (int64_t)s->nodes.size();
        int64_t leaves = 0, nonempty = 0;
        for (const NodeRec &nr : s->nodes) {
                if (nr.a & kLeafBit) {
                        ++leaves;
                        if (nr.a & ~kLeafBit)
                                ++nonempty;
                }
        }
        s->wide_leaves = refs.size() >= 8 * (size_t)std::max<int64_t>(1, nonempty);
        s->ref_tri.resize(refs.size());
        if (s->wide_leaves)
                s->refs64.resize(refs.size());
        else
                s->refs48.resize(refs.size());
        for (size_t i = 0; i < refs.size(); ++i) {
                const uint32_t t = (uint32_t)(refs[i] & 0xFFFFFFFFu);
                s->ref_tri[i] = t;
                const float *p = d->pos + 9 * (size_t)t;
                if (s->wide_leaves) {
                        RefRec64 &rr = s->refs64[i];
                        for (int k = 0; k < 3; ++k) {
                                rr.v0[k] = p[k];
                                rr.e1[k] = (double)p[3 + k] - (double)p[k];  // SUB(edge1, vert1, vert0)
                                rr.e2[k] = (double)p[6 + k] - (double)p[k];  // SUB(edge2, vert2, vert0)
                        }
                        rr.tri = t;
                } else {
                        RefRec48 &rr = s->refs48[i];
                        std::memcpy(rr.p, p, sizeof rr.p);
                        rr.tri = t;
                        rr.pad[0] = rr.pad[1] = 0;
                }
        }
        s->info.nodes = nnodes;
        s->info.internal = ninternal;
        s->info.leaves = leaves;
        s->info.nonempty_leaves = nonempty;
        s->info.tri_refs = (int64_t)refs.size();
        for (int k = 0; k < 3; ++k) {
                s->info.root_min[k] = root.mn[k];
                s->info.root_max[k] = root.mx[k];
        }
        return VRT_OK;
}

static int check_device(int device)
{
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
                return fail(VRT_E_NODEVICE, "no HIP device visible");
        if (device < 0 || device >= n)
                return fail(VRT_E_NODEVICE, "device %d out of range (%d visible)", device, n);
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, device));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
                return fail(VRT_E_NODEVICE, "device %d is %s, kernels are built for gfx950",
                            device, prop.gcnArchName);
        return VRT_OK;
}

extern "C" int vrt_device_count(int *n)
{
        if (!n)
                return fail(VRT_E_INVALID, "null");
        *n = 0;
        int c = 0;
        if (hipGetDeviceCount(&c) != hipSuccess)
                return VRT_OK;
        *n = c;
        return VRT_OK;
}

static size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// DevScene::xnodes: every node's own record followed by the union box of all
// triangles below it (a leaf: its own), enlarged by eps = 2^-16 * the root's
// largest extent and rounded outward to float.  Sets lb_center and
// lb_reach = 16 * that extent: for a ray origin within lb_reach of the
// centre (per axis) and a point of a leaf's triangles, every slab distance
// |p - o| / |d| is below 17 * extent / |d|, the three fp32 roundings of
// (p - o) * (1/d) move it by less than 3 * 2^-24 * 17 * extent / |d| <
// eps / |d|, so the fp32 line test on the enlarged box passes whenever the
// exact line meets the unenlarged one -- and intersect_triangle3 accepts a
// triangle only where the line meets it (up to its fp64 rounding, far below
// eps); an internal node's box bounds the triangles of its leaves, which all
// lie in the root box, so the same bound holds.  Nodes with no triangle below
// them (never visited by the content-masked walk), and every node of a scene
// whose extent is not finite and positive (no skip), carry their voxel box.
static void march_nodes(vrt_scene *s, const vrt_scene_desc *d, std::vector<XNodeRec> &xn);

// The float box [l - eps, h + eps] rounded outward: the one enlargement of a
// triangle box, shared by DevScene::xnodes and the per-record boxes (RefBox).
static void enlarged_box(const double l[3], const double h[3], double eps, float bl[3], float bh[3])
{
        for (int k = 0; k < 3; ++k) {
                float fl = (float)(l[k] - eps), fh = (float)(h[k] + eps);
                if ((double)fl > l[k] - eps)
                        fl = std::nextafter(fl, -HUGE_VALF);
                if ((double)fh < h[k] + eps)
                        fh = std::nextafter(fh, HUGE_VALF);
                bl[k] = fl;
                bh[k] = fh;
        }
}

// The root box's largest extent: lb_eps = 2^-16 * it, and the skips are on
// (lb_reach >= 0) only when it is finite and positive.
static float scene_extent(const vrt_scene *s)
{
        float ext = 0.f;
        for (int k = 0; k < 3; ++k)
                ext = std::max(ext, s->info.root_max[k] - s->info.root_min[k]);
        return ext;
}

// Does the scene carry the per-record boxes (RefBox, vrt_internal.h)?
static bool has_ref_boxes(const vrt_scene *s)
{
        const float ext = scene_extent(s);
        return VRT_LEAF_CULL && !s->wide_leaves && ext > 0.f && std::isfinite(ext);
}

// The per-record boxes in device order: out[n - 1 - j] = the box of record
// j's triangle, the box march_nodes gives a leaf holding that triangle alone
// (a triangle with a NaN coordinate gets the inverted infinite box, which
// the line test keeps; intersect_triangle3 then rejects it as it always
// does).  Only for has_ref_boxes() scenes.
static void ref_boxes(const vrt_scene *s, const vrt_scene_desc *d, std::vector<RefBox> &out)
{
        const size_t n = s->ref_tri.size();
        const double eps = std::ldexp((double)scene_extent(s), -16);
        out.resize(n);
        for (size_t j = 0; j < n; ++j) {
                const float *p = d->pos + 9 * (size_t)s->ref_tri[j];
                double l[3] = { HUGE_VAL, HUGE_VAL, HUGE_VAL }, h[3] = { -HUGE_VAL, -HUGE_VAL, -HUGE_VAL };
                bool nan = false;
                for (int v = 0; v < 3; ++v)
                        for (int k = 0; k < 3; ++k) {
                                nan = nan || std::isnan(p[3 * v + k]);
                                l[k] = std::min(l[k], (double)p[3 * v + k]);
                                h[k] = std::max(h[k], (double)p[3 * v + k]);
                        }
                RefBox rb{};
                if (nan) {
                        for (int k = 0; k < 3; ++k) {
                                rb.bmin[k] = HUGE_VALF;
                                rb.bmax[k] = -HUGE_VALF;
                        }
                } else {
                        enlarged_box(l, h, eps, rb.bmin, rb.bmax);
                }
                out[n - 1 - j] = rb;
        }
}

static void march_nodes(vrt_scene *s, const vrt_scene_desc *d, std::vector<XNodeRec> &xn)
{
        const size_t nn = s->nodes.size();
        xn.resize(nn);
        for (size_t i = 0; i < nn; ++i) {
                xn[i] = XNodeRec{};
                xn[i].n = s->nodes[i];
                for (int k = 0; k < 3; ++k) {
                        xn[i].tmin[k] = s->nodes[i].bmin[k];
                        xn[i].tmax[k] = s->nodes[i].bmax[k];
                }
        }
        const float ext = scene_extent(s);
        for (int k = 0; k < 3; ++k)
                s->dev.lb_center[k] = 0.5f * (s->info.root_min[k] + s->info.root_max[k]);
        s->dev.lb_reach = 16.f * ext;
        if (!(ext > 0.f) || !std::isfinite(ext)) {
                s->dev.lb_reach = -1.f;  // never skip
                return;
        }
        const double eps = std::ldexp((double)ext, -16);
        // unenlarged triangle boxes, bottom-up (children follow their parent
        // in the BFS array)
        std::vector<double> lo(3 * nn, HUGE_VAL), hi(3 * nn, -HUGE_VAL);
        for (size_t i = nn; i-- > 0;) {
                const NodeRec &nr = s->nodes[i];
                double *l = &lo[3 * i], *h = &hi[3 * i];
                if (nr.a & kLeafBit) {
                        const uint32_t n = nr.a & ~kLeafBit;
                        for (uint32_t j = 0; j < n; ++j) {
                                const float *p = d->pos + 9 * (size_t)s->ref_tri[nr.b + j];
                                for (int v = 0; v < 3; ++v)
                                        for (int k = 0; k < 3; ++k) {
                                                l[k] = std::min(l[k], (double)p[3 * v + k]);
                                                h[k] = std::max(h[k], (double)p[3 * v + k]);
                                        }
                        }
                } else {
                        for (uint32_t c = 0; c < 8; ++c)
                                for (int k = 0; k < 3; ++k) {
                                        l[k] = std::min(l[k], lo[3 * (nr.a + c) + k]);
                                        h[k] = std::max(h[k], hi[3 * (nr.a + c) + k]);
                                }
                }
        }
        for (size_t i = 1; i < nn; ++i) {
                const double *l = &lo[3 * i], *h = &hi[3 * i];
                if (!(l[0] <= h[0]))
                        continue;  // no triangle below this node
                enlarged_box(l, h, eps, xn[i].tmin, xn[i].tmax);
        }
}

// vrt_scene::ord_wmin: per axis the minimum over the internal nodes of
// cm[k][1] - cm[k][0], the child centres exactly as expand_v2 makes them
// (float operations, no contraction), the difference taken in double (exact)
// and rounded down to float.  All zero (the chain order is off) unless the
// scene is fast_ok, every value is finite and positive and every centre lies
// in the root box (the bound |centre - o| <= R_k of chain_criterion).
static void chain_spacing(vrt_scene *s)
{
        for (int k = 0; k < 3; ++k)
                s->ord_wmin[k] = 0.f;
        if (!s->dev.fast_ok || s->nodes.empty())
                return;
        double w[3] = { HUGE_VAL, HUGE_VAL, HUGE_VAL };
        bool any = false, ok = true;
        const NodeRec &root = s->nodes[0];
        for (const NodeRec &nr : s->nodes) {
                if (nr.a & kLeafBit)
                        continue;
                any = true;
                for (int k = 0; k < 3; ++k) {
                        const float h = (nr.bmax[k] - nr.bmin[k]) / 2.0f;
                        const float a0 = nr.bmin[k];
                        const float b = nr.bmin[k] + h;
                        const float c = b + h;
                        const float c0 = (a0 + b) * .5f;
                        const float c1 = (b + c) * .5f;
                        w[k] = std::min(w[k], (double)c1 - (double)c0);
                        ok = ok && c0 >= root.bmin[k] && c0 <= root.bmax[k] && c1 >= root.bmin[k] &&
                             c1 <= root.bmax[k];  // false for NaN
                }
        }
        float f[3];
        for (int k = 0; k < 3; ++k) {
                ok = ok && any && std::isfinite(w[k]) && w[k] > 0.0;
                f[k] = (float)w[k];
                if (ok && (double)f[k] > w[k])
                        f[k] = std::nextafter(f[k], 0.f);
                ok = ok && f[k] > 0.f;
        }
        if (ok)
                for (int k = 0; k < 3; ++k)
                        s->ord_wmin[k] = f[k];
}

static int upload(vrt_scene *s, const vrt_scene_desc *d)
{
        int rc = check_device(s->device);
        if (rc)
                return rc;
        HIPCHK(hipSetDevice(s->device));
        const size_t sz_nodes = s->nodes.size() * sizeof(NodeRec);
        const size_t sz_vox = s->node_vox.size() * sizeof(uint32_t);
        const void *refs_host = s->wide_leaves ? (const void *)s->refs64.data() : (const void *)s->refs48.data();
        const size_t refs_bytes = s->wide_leaves ? s->refs64.size() * sizeof(RefRec64)
                                                 : s->refs48.size() * sizeof(RefRec48);
        // the per-record boxes lie directly below the records (RefBox): the
        // region is [pad | boxes, last record's first | records]
        const bool rboxes = has_ref_boxes(s);
        const size_t sz_rbox = rboxes ? align_up((s->ref_tri.size() + kRefBoxPad) * sizeof(RefBox)) : 0;
        const size_t sz_refs = sz_rbox + std::max<size_t>(64, refs_bytes);
        const size_t sz_pos = std::max<size_t>(1, s->tri_pos.size()) * sizeof(TriPos);
        const size_t sz_attr = std::max<size_t>(1, s->tri_attr.size()) * sizeof(TriAttr);
        const size_t sz_mats = s->mats.size() * sizeof(MatRec);
        const size_t sz_texs = std::max<size_t>(1, s->texs.size()) * sizeof(TexRec);
        const size_t sz_tex = (size_t)std::max<int64_t>(16, s->tex_bytes);
        size_t off[11];
        size_t tot = 0, fixed = 0;
        const size_t sz_xnodes = s->nodes.size() * sizeof(XNodeRec);
        const size_t sizes[10] = { sz_nodes, sz_vox, sz_refs, sz_pos, sz_attr, sz_mats, sz_texs, sz_tex,
                                   kQueueSlots * kQueueBytes, sz_xnodes };
        // regions 0, 1, 2 and 9 follow the geometry (their own owners); the
        // rest share d_mem.  device_bytes counts all ten as it always has.
        for (int i = 0; i < 10; ++i) {
                const bool geo = i <= 2 || i == 9;
                off[i] = geo ? 0 : fixed;
                tot += align_up(sizes[i]);
                if (!geo)
                        fixed += align_up(sizes[i]);
        }
        off[10] = tot;
        HIPCHK(s->d_mem.alloc(fixed));
        HIPCHK(s->g_nodes.alloc(align_up(sz_nodes)));
        HIPCHK(s->g_vox.alloc(align_up(sz_vox)));
        HIPCHK(s->g_refs.alloc(align_up(sz_refs)));
        HIPCHK(s->g_xnodes.alloc(align_up(sz_xnodes)));
        s->rboxes = rboxes;
        char *base = s->d_mem.as<char>();
        HIPCHK(hipMemset(base + off[8], 0, kQueueSlots * kQueueBytes));
        HIPCHK(hipMemcpy(s->g_nodes, s->nodes.data(), sz_nodes, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(s->g_vox, s->node_vox.data(), sz_vox, hipMemcpyHostToDevice));
        if (refs_bytes)
                HIPCHK(hipMemcpy(s->g_refs.as<char>() + sz_rbox, refs_host, refs_bytes, hipMemcpyHostToDevice));
        if (!s->tri_pos.empty())
                HIPCHK(hipMemcpy(base + off[3], s->tri_pos.data(), s->tri_pos.size() * sizeof(TriPos), hipMemcpyHostToDevice));
        if (!s->tri_attr.empty())
                HIPCHK(hipMemcpy(base + off[4], s->tri_attr.data(), s->tri_attr.size() * sizeof(TriAttr), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(base + off[5], s->mats.data(), sz_mats, hipMemcpyHostToDevice));
        if (!s->texs.empty())
                HIPCHK(hipMemcpy(base + off[6], s->texs.data(), s->texs.size() * sizeof(TexRec), hipMemcpyHostToDevice));
        if (s->tex_bytes > 0)
                HIPCHK(hipMemcpy(base + off[7], d->tex_data, (size_t)s->tex_bytes, hipMemcpyHostToDevice));
        s->dev.nodes = s->g_nodes.as<NodeRec>();
        s->dev.node_vox = s->g_vox.as<uint32_t>();
        s->dev.refs = s->g_refs.as<char>() + sz_rbox;
        s->dev.tri_pos = reinterpret_cast<const TriPos *>(base + off[3]);
        s->dev.tri_attr = reinterpret_cast<const TriAttr *>(base + off[4]);
        s->dev.mats = reinterpret_cast<const MatRec *>(base + off[5]);
        s->dev.texs = reinterpret_cast<const TexRec *>(base + off[6]);
        s->dev.tex_data = reinterpret_cast<const uint8_t *>(base + off[7]);
        s->d_queue = reinterpret_cast<uint32_t *>(base + off[8]);
        {
                // the march records of the nodes (DevScene::xnodes)
                std::vector<XNodeRec> xn;
                march_nodes(s, d, xn);
                if (sz_xnodes)
                        HIPCHK(hipMemcpy(s->g_xnodes, xn.data(), sz_xnodes, hipMemcpyHostToDevice));
                s->dev.xnodes = s->g_xnodes.as<XNodeRec>();
        }
        if (rboxes && !s->ref_tri.empty()) {
                std::vector<RefBox> rb;
                ref_boxes(s, d, rb);
                const size_t nb = rb.size() * sizeof(RefBox);
                HIPCHK(hipMemcpy(s->g_refs.as<char>() + sz_rbox - nb, rb.data(), nb, hipMemcpyHostToDevice));
        }
        HIPCHK(persistent_blocks(&s->dev.persist_blocks, &s->dev.sec_blocks));
        s->dev.grid_div = 1;
        s->dev.max_depth = s->max_depth;
        s->dev.nmat = (int32_t)s->mats.size();
        s->dev.ntex = (int32_t)s->texs.size();
        {
                bool ok = true;
                for (int k = 0; k < 3; ++k) {
                        const float lo = s->info.root_min[k], hi = s->info.root_max[k];
                        ok = ok && std::fabs(lo) < 0x1p60f && std::fabs(hi) < 0x1p60f;  // see fast_ok()
                }
                s->dev.fast_ok = ok ? 1 : 0;
                s->dev.wide_leaves = s->wide_leaves ? 1 : 0;
        }
        chain_spacing(s);
        if (!s->probes.empty()) {
                // probe membership beside the octree (ProbeDev): DevScene's
                // layout is untouched
                static_assert(sizeof(vrt_probe) == sizeof(float4), "vrt_probe layout");
                const size_t sz_pn = align_up(s->pnode.size() * sizeof(uint2));
                const size_t sz_pr = align_up(std::max<size_t>(1, s->pref.size()) * sizeof(uint32_t));
                const size_t sz_pb = align_up(s->probes.size() * sizeof(vrt_probe));
                const size_t sz_sg = align_up(s->probe_sgs.size() * sizeof(vrt_sg));
                HIPCHK(s->g_pnode.alloc(sz_pn));
                HIPCHK(s->g_pref.alloc(sz_pr));
                HIPCHK(s->d_probe.alloc(sz_pb + sz_sg));
                char *pb = s->d_probe.as<char>();
                HIPCHK(hipMemcpy(s->g_pnode, s->pnode.data(), s->pnode.size() * sizeof(uint2), hipMemcpyHostToDevice));
                if (!s->pref.empty())
                        HIPCHK(hipMemcpy(s->g_pref, s->pref.data(), s->pref.size() * sizeof(uint32_t),
                                         hipMemcpyHostToDevice));
                HIPCHK(hipMemcpy(pb, s->probes.data(), s->probes.size() * sizeof(vrt_probe), hipMemcpyHostToDevice));
                s->pdev.pnode = s->g_pnode.as<uint2>();
                s->pdev.pref = s->g_pref.as<uint32_t>();
                s->pdev.probes = reinterpret_cast<const float4 *>(pb);
                s->pdev.ntri = s->ntri;
                s->d_sgs = reinterpret_cast<float *>(pb + sz_pb);
                HIPCHK(hipMemcpy(s->d_sgs, s->probe_sgs.data(), s->probe_sgs.size() * sizeof(vrt_sg),
                                 hipMemcpyHostToDevice));
                tot += sz_pn + sz_pr + sz_pb + sz_sg;
        }
        s->info.device_bytes = (int64_t)tot;
        HIPCHK(s->stream.create());
        HIPCHK(s->ev0.create());
        HIPCHK(s->ev1.create());
        for (LastUse &q : s->q_use)
                HIPCHK(q.create());
        for (TraceSet &t : s->ts)
                HIPCHK(t.use.create());
        return VRT_OK;
}

static int validate_desc(const vrt_scene_desc *d, int max_depth)
{
        if (!d)
                return fail(VRT_E_INVALID, "null scene descriptor");
        if (max_depth < 1 || max_depth > VRT_MAX_DEPTH)
                return fail(VRT_E_INVALID, "max_depth %d outside [1,%d]", max_depth, VRT_MAX_DEPTH);
        if (d->ntri < 0 || (d->ntri > 0 && (!d->pos || !d->nrm)))
                return fail(VRT_E_INVALID, "bad triangle arrays");
        if (d->nmat < 1 || !d->mat_tex || !d->mat_kd)
                return fail(VRT_E_INVALID, "need >= 1 material (mat_tex, mat_kd)");
        if (d->ntex < 0 || (d->ntex > 0 && (!d->tex_dims || !d->tex_off || !d->tex_data)))
                return fail(VRT_E_INVALID, "bad texture arrays");
        for (int m = 0; m < d->nmat; ++m)
                if (d->mat_tex[m] < -1 || d->mat_tex[m] >= d->ntex)
                        return fail(VRT_E_INVALID, "material %d: texture id %d out of range", m, d->mat_tex[m]);
        for (int t = 0; t < d->ntex; ++t) {
                const int w = d->tex_dims[3 * t], h = d->tex_dims[3 * t + 1], c = d->tex_dims[3 * t + 2];
                if (w < 1 || h < 1 || c < 1 || c > 4 || d->tex_off[t] < 0 ||
                    d->tex_off[t] + (int64_t)w * h * c > d->tex_bytes)
                        return fail(VRT_E_INVALID, "texture %d: bad dims/offset", t);
        }
        if (d->mat)
                for (int i = 0; i < d->ntri; ++i)
                        if (d->mat[i] < 0 || d->mat[i] >= d->nmat)
                                return fail(VRT_E_INVALID, "triangle %d: material %d out of range", i, d->mat[i]);
        return VRT_OK;
}

extern "C" int vrt_scene_create(const vrt_scene_desc *d, int max_depth,
                                int device, vrt_scene **out)
{
        return vrt_scene_create_ex(d, max_depth, device, 0, out);
}

static int scene_create(const vrt_scene_desc *d, const vrt_probe *probes, int32_t nprobe, int max_depth,
                        int device, int flags, vrt_scene **out);

extern "C" int vrt_scene_create_ex(const vrt_scene_desc *d, int max_depth,
                                   int device, int flags, vrt_scene **out)
{
        return scene_create(d, nullptr, 0, max_depth, device, flags, out);
}

extern "C" int vrt_scene_create_probes(const vrt_scene_desc *d, const vrt_probe *probes, int32_t nprobe,
                                       int max_depth, int device, int flags, vrt_scene **out)
{
        if (nprobe == 0 || !probes)
                return scene_create(d, nullptr, 0, max_depth, device, flags, out);
        return scene_create(d, probes, nprobe, max_depth, device, flags, out);
}

static int scene_create(const vrt_scene_desc *d, const vrt_probe *probes, int32_t nprobe, int max_depth,
                        int device, int flags, vrt_scene **out)
{
        if (!out)
                return fail(VRT_E_INVALID, "null out");
        *out = nullptr;
        int rc = validate_desc(d, max_depth);
        if (rc)
                return rc;
        if (flags & ~(VRT_BUILD_DEVICE | VRT_BUILD_DEVICE_PROBES))
                return fail(VRT_E_INVALID, "unknown flags %#x", flags);
        if ((flags & VRT_BUILD_DEVICE_PROBES) && !(flags & VRT_BUILD_DEVICE))
                return fail(VRT_E_INVALID, "VRT_BUILD_DEVICE_PROBES goes with VRT_BUILD_DEVICE (flags %#x)", flags);
        if ((flags & VRT_BUILD_DEVICE) && device < 0)
                return fail(VRT_E_INVALID, "VRT_BUILD_DEVICE needs a device (device >= 0)");
        if (probes) {
                if (nprobe < 1 || (int64_t)d->ntri + (int64_t)nprobe > 0x7FFFFFFF)
                        return fail(VRT_E_INVALID, "bad probe count %d (ntri + nprobe must stay below 2^31)", nprobe);
                if ((flags & VRT_BUILD_DEVICE) && !(flags & VRT_BUILD_DEVICE_PROBES))
                        return fail(VRT_E_INVALID, "VRT_BUILD_DEVICE alone inserts triangles only: add "
                                                   "VRT_BUILD_DEVICE_PROBES to build a probe scene on the device");
                for (int32_t k = 0; k < nprobe; ++k) {
                        const vrt_probe &pb = probes[k];
                        if (!std::isfinite(pb.o[0]) || !std::isfinite(pb.o[1]) || !std::isfinite(pb.o[2]) ||
                            !std::isfinite(pb.r) || pb.r < 0.f)
                                return fail(VRT_E_INVALID, "probe %d: centre must be finite, radius finite and >= 0", k);
                }
        }
        std::unique_ptr<vrt_scene> s(new (std::nothrow) vrt_scene);
        if (!s)
                return fail(VRT_E_NOMEM, "scene alloc");
        s->device = device;
        s->max_depth = max_depth;
        s->ntri = d->ntri;
        const double t0 = now_ms();
        try {
                if (probes) {
                        s->probes.assign(probes, probes + nprobe);
                        s->probe_sgs.assign((size_t)kProbeSGs * (size_t)nprobe, vrt_sg{});
                }
                rc = build_tree(s.get(), d, (flags & VRT_BUILD_DEVICE) != 0);
                if (rc)
                        return rc;
                const int n = d->ntri;
                s->tri_pos.resize((size_t)n);
                s->tri_attr.resize((size_t)n);
                for (int i = 0; i < n; ++i) {
                        TriPos &tp = s->tri_pos[i];
                        std::memcpy(tp.p, d->pos + 9 * (size_t)i, sizeof tp.p);
                        tp.pad[0] = tp.pad[1] = tp.pad[2] = 0.f;
                        TriAttr &ta = s->tri_attr[i];
                        for (int v = 0; v < 3; ++v) {
                                const float *nn = d->nrm + 9 * (size_t)i + 3 * v;
                                const f3 q = normalize(mk3(nn[0], nn[1], nn[2]));
                                ta.n[3 * v + 0] = q.x;
                                ta.n[3 * v + 1] = q.y;
                                ta.n[3 * v + 2] = q.z;
                        }
                        for (int k = 0; k < 6; ++k)
                                ta.t[k] = d->uv ? d->uv[6 * (size_t)i + k] : 0.f;
                        ta.mat = d->mat ? d->mat[i] : 0;
                }
                s->mats.resize((size_t)d->nmat);
                for (int m = 0; m < d->nmat; ++m) {
                        s->mats[m].tex = d->mat_tex[m];
                        for (int k = 0; k < 3; ++k)
                                s->mats[m].kd[k] = d->mat_kd[3 * m + k];
                }
                s->texs.resize((size_t)d->ntex);
                for (int t = 0; t < d->ntex; ++t) {
                        s->texs[t].off = d->tex_off[t];
                        s->texs[t].w = d->tex_dims[3 * t];
                        s->texs[t].h = d->tex_dims[3 * t + 1];
                        s->texs[t].c = d->tex_dims[3 * t + 2];
                        s->texs[t].pad = 0;
                }
                for (auto &mr : s->mats)
                        mr.tx = (mr.tex >= 0 && mr.tex < d->ntex) ? s->texs[(size_t)mr.tex] : TexRec{};
                s->tex_bytes = d->ntex ? d->tex_bytes : 0;
        } catch (const std::bad_alloc &) {
                return fail(VRT_E_NOMEM, "octree build: out of host memory");
        }
        s->info.build_ms = now_ms() - t0;
        s->info.max_depth = max_depth;
        s->info.device = device;
        const double t1 = now_ms();
        if (device < 0) {  // host-only scene: build and inspect, no device
                *out = s.release();
                return VRT_OK;
        }
        rc = upload(s.get(), d);
        if (rc) {
                vrt_scene_destroy(s.release());
                return rc;
        }
        s->info.upload_ms = now_ms() - t1;
        *out = s.release();
        return VRT_OK;
}

// The same scene on another device (vrt_scene_create_multi): the host-side
// octree, leaf records and shading tables of `src` are copied, not rebuilt,
// and uploaded to `device` exactly as vrt_scene_create uploads them.
int vrt::scene_replicate(const vrt_scene *src, const vrt_scene_desc *d, int device, vrt_scene **out)
{
        *out = nullptr;
        std::unique_ptr<vrt_scene> s(new (std::nothrow) vrt_scene);
        if (!s)
                return fail(VRT_E_NOMEM, "scene alloc");
        const double t0 = now_ms();
        try {
                s->device = device;
                s->max_depth = src->max_depth;
                s->ntri = src->ntri;
                s->nodes = src->nodes;
                s->node_vox = src->node_vox;
                s->refs48 = src->refs48;
                s->refs64 = src->refs64;
                s->wide_leaves = src->wide_leaves;
                s->ref_tri = src->ref_tri;
                s->tri_pos = src->tri_pos;
                s->tri_attr = src->tri_attr;
                s->mats = src->mats;
                s->texs = src->texs;
                s->tex_bytes = src->tex_bytes;
                s->info = src->info;
                s->level_begin = src->level_begin;
                // a probe scene's probes, per-node probe lists and masks, leaf
                // lists and stored SGs (upload() makes their device copy)
                s->probes = src->probes;
                s->pnode = src->pnode;
                s->pref = src->pref;
                s->probe_sgs = src->probe_sgs;
                s->probe_leaves = src->probe_leaves;
        } catch (const std::bad_alloc &) {
                return fail(VRT_E_NOMEM, "scene replica: out of host memory");
        }
        s->info.device = device;
        s->info.build_ms = 0;
        if (int rc = upload(s.get(), d)) {
                vrt_scene_destroy(s.release());
                return rc;
        }
        s->info.upload_ms = now_ms() - t0;
        *out = s.release();
        return VRT_OK;
}

// The owners release everything; what is left to do first is to wait for the
// scene's work in flight.  A scene that was never uploaded (host-only: no
// d_mem, need_device) holds nothing and touches no device.
extern "C" void vrt_scene_destroy(vrt_scene *s)
{
        if (!s)
                return;
        if (s->d_mem) {
                (void)hipSetDevice(s->device);
                if (s->stream)
                        (void)hipStreamSynchronize(s->stream);
                // launches on callers' streams: every work-queue slot, trace
                // set, compaction set and deal map records its last user's event
                for (LastUse &q : s->q_use)
                        (void)q.sync();
                for (TraceSet &t : s->ts)
                        (void)t.use.sync();
                for (LastUse &u : s->spill_use)
                        (void)u.sync();
                for (auto &m : s->dmaps)
                        (void)m.built.sync();
                if (s->ho.st2)
                        (void)hipStreamSynchronize(s->ho.st2);
                if (s->ho.cp)
                        (void)hipStreamSynchronize(s->ho.cp);
        }
        delete s;
}

void vrt::scene_mark_owned(vrt_scene *s) { s->owned = true; }

extern "C" int vrt_scene_info(const vrt_scene *s, vrt_scene_info_t *info)
{
        if (!s || !info)
                return fail(VRT_E_INVALID, "null argument");
        *info = s->info;
        return VRT_OK;
}

extern "C" int vrt_scene_ref_format(const vrt_scene *s, int32_t *record_bytes)
{
        if (!s || !record_bytes)
                return fail(VRT_E_INVALID, "null argument");
        *record_bytes = s->wide_leaves ? (int32_t)sizeof(RefRec64) : (int32_t)sizeof(RefRec48);
        return VRT_OK;
}

extern "C" int vrt_scene_nodes(const vrt_scene *s, float *box, uint32_t *a, uint32_t *b)
{
        if (!s)
                return fail(VRT_E_INVALID, "null argument");
        for (size_t i = 0; i < s->nodes.size(); ++i) {
                const NodeRec &nr = s->nodes[i];
                if (box) {
                        std::memcpy(box + 6 * i, nr.bmin, 12);
                        std::memcpy(box + 6 * i + 3, nr.bmax, 12);
                }
                if (a)
                        a[i] = nr.a;
                if (b)
                        b[i] = nr.b;
        }
        return VRT_OK;
}

extern "C" int vrt_scene_leaves(const vrt_scene *s, uint32_t *voxel,
                                uint32_t *count, int32_t *tris)
{
        if (!s || !voxel || !count || !tris)
                return fail(VRT_E_INVALID, "null argument");
        std::vector<std::pair<uint32_t, size_t>> lv;
        for (size_t i = 0; i < s->nodes.size(); ++i) {
                const NodeRec &nr = s->nodes[i];
                if ((nr.a & kLeafBit) && (nr.a & ~kLeafBit))
                        lv.emplace_back(s->node_vox[i], i);
        }
        std::sort(lv.begin(), lv.end());
        size_t o = 0;
        for (size_t j = 0; j < lv.size(); ++j) {
                const NodeRec &nr = s->nodes[lv[j].second];
                const uint32_t n = nr.a & ~kLeafBit;
                voxel[j] = lv[j].first;
                count[j] = n;
                for (uint32_t k = 0; k < n; ++k)
                        tris[o++] = (int32_t)s->ref_tri[nr.b + k];
        }
        return VRT_OK;
}

// ---------------------------------------------------------------------------
// render
// ---------------------------------------------------------------------------
static int need_device(const vrt_scene *s)
{
        if (!s->d_mem)
                return fail(VRT_E_NODEVICE, "scene was created host-only (device < 0)");
        return VRT_OK;
}

// The film kernels of trace() and the instrumented render count or march
// as the reference does with every voxel in the tree; they do not know probe
// voxels yet (a follow-up).
static int no_probe_scene(const vrt_scene *s, const char *what)
{
        if (!s->probes.empty())
                return fail(VRT_E_INVALID,
                            "%s is not available on a scene with light probes; use vrt_trace_batch for its rays", what);
        return VRT_OK;
}

static int film_ok(const vrt_film *f)
{
        if (!f || f->nx < 1 || f->ny < 1 || f->nx > 32768 || f->ny > 32768)
                return fail(VRT_E_INVALID, "bad film");
        return VRT_OK;
}

extern "C" int vrt_tiles_per_rank(const vrt_film *film, int nranks)
{
        if (film_ok(film) || nranks < 1)
                return 0;
        // the largest share of the tile deal (tile_deal, vrt_internal.h)
        const TileDeal d = tile_deal(film->nx / 8, film->ny / 8, nranks);
        int m = 0;
        for (int r = 0; r < nranks; ++r)
                m = std::max(m, deal_count(d, r));
        return m;
}

extern "C" int vrt_scene_set_frames_in_flight(vrt_scene *s, int n)
{
        if (!s || n < 1)
                return fail(VRT_E_INVALID, "bad argument");
        std::lock_guard<std::mutex> lk(s->mu);
        // measured: half the slots per frame with 2-3 frames
        // in flight; a third is slower, the whole chip per frame the same
        // (round 6, bench's own schedule)
        s->dev.grid_div = n >= 2 ? 2 : 1;
        return VRT_OK;
}

extern "C" int vrt_tile_deal_block(void)
{
        return VRT_DEAL_BLOCK;
}

extern "C" int vrt_tile_deal_map(const vrt_film *film, int nranks, int32_t *rank_of_tile, int32_t *slot_of_tile)
{
        if (int rc = film_ok(film))
                return rc;
        if (nranks < 1 || !rank_of_tile || !slot_of_tile)
                return fail(VRT_E_INVALID, "bad argument");
        const int ntx = film->nx / 8, nty = film->ny / 8;
        const TileDeal d = tile_deal(ntx, nty, nranks);
        for (int ty = 0; ty < nty; ++ty)
                for (int tx = 0; tx < ntx; ++tx) {
                        int r, k;
                        deal_slot(d, tx, ty, r, k);
                        rank_of_tile[ty * ntx + tx] = r;
                        slot_of_tile[ty * ntx + tx] = k;
                        // the forward map must invert it
                        int bx = -1, by = -1;
                        if (k < deal_count(d, r))
                                deal_tile(d, r, k, bx, by);
                        if (bx != tx || by != ty)
                                return fail(VRT_E_INVALID, "tile deal does not invert at (%d, %d)", tx, ty);
                }
        return VRT_OK;
}

static std::atomic<int> g_test_flags{0};

extern "C" int vrt_set_test_flags(int flags)
{
        g_test_flags.store(flags);
        return VRT_OK;
}

int vrt::test_flags() { return g_test_flags.load(); }

extern "C" int vrt_test_flags(void) { return g_test_flags.load(); }

extern "C" int vrt_build_flag(const char *name, int64_t *value)
{
        if (!name || !value)
                return fail(VRT_E_INVALID, "null argument");
        if (std::strcmp(name, "VRT_DIGEST_PASS_WORDS") == 0) {  // vrt_digest.hip
                *value = digest_pass_words();
                return VRT_OK;
        }
        if (!build_flag(name, value))
                return fail(VRT_E_INVALID, "unknown build flag %s", name);
        return VRT_OK;
}

static void fill_render_params(vrt_scene *s, const vrt_camera *cam,
                               const vrt_film *film, int rank, int nranks,
                               RenderParams *p)
{
        std::memset(p, 0, sizeof *p);
        p->sc = s->dev;
        fill_cam_params(cam, film, &p->cam);
        p->ntx = film->nx / 8;
        p->nty = film->ny / 8;
        p->rank = rank;
        p->nranks = nranks;
        p->tiles_this_rank = deal_count(tile_deal(p->ntx, p->nty, nranks), rank);
        // k * ceil(2^40 / ntx) >> 40 == k / ntx for k < 2^40 / ntx, which
        // k < 2^24 and ntx < 2^16 guarantee
        if (p->ntx > 0 && p->ntx < (1 << 16) && (int64_t)p->ntx * p->nty < ((int64_t)1 << 24))
                p->ntx_magic = (((uint64_t)1 << 40) + (uint64_t)p->ntx - 1) / (uint64_t)p->ntx;
        p->test_flags = g_test_flags.load();
}

static float scene_res(const vrt_scene *s);

// Work-queue ring (WorkQueue, vrt_internal.h; caller holds s->mu).  A
// persistent launch takes the next slot: its stream first waits for the
// slot's previous launch (on whatever stream it ran), the kernel takes its
// units from base[] on, and the slot's bases advance by exactly the adds the
// launch makes.
static int queue_take(vrt_scene *s, hipStream_t st, WorkQueue *q, int *slot)
{
        *slot = s->q_next;
        s->q_next = (*slot + 1) % kQueueSlots;
        HIPCHK(s->q_use[*slot].wait(st));
        q->ctr = s->d_queue + (size_t)*slot * kQueueWords;
        q->defer = q->ctr + 8 * kQueueStride;
        std::memcpy(q->base, s->q_base[*slot], sizeof q->base);
        return VRT_OK;
}

static int queue_release(vrt_scene *s, int slot, hipStream_t st, const int slice_units[8], int waves)
{
        for (int x = 0; x < 8; ++x)
                if (slice_units[x] > 0)
                        s->q_base[slot][x] += (uint32_t)slice_units[x] + (uint32_t)waves;
        HIPCHK(s->q_use[slot].record(st));
        return VRT_OK;
}

// A launch failed after taking `slot`: whatever part of it was enqueued runs
// before this memset (same stream), then the slot restarts from zero
// counters, zero bases and an empty deferred list -- so a failed launch
// never leaves a slot whose bases disagree with its counters (every later
// launch on it would otherwise find its queue already drained).
static void queue_reset(vrt_scene *s, int slot, hipStream_t st)
{
        (void)hipMemsetAsync(s->d_queue + (size_t)slot * kQueueWords, 0, kQueueBytes, st);
        std::memset(s->q_base[slot], 0, sizeof s->q_base[slot]);
        (void)s->q_use[slot].record(st);
}

// One render launch on stream st (caller holds s->mu).
static int render_launch(vrt_scene *s, RenderParams &p, bool instrumented, hipStream_t st)
{
        int slot = -1;
        (void)hipGetLastError();  // a leftover error of an earlier call is not this launch's
        if (render_kind(p, instrumented) != kRenderGrid) {
                if (int rc = queue_take(s, st, &p.q, &slot))
                        return rc;
        }
        int waves = 0, units[8];
        uint32_t *entry = nullptr;
        hipError_t e = hipSuccess;
        if (slot >= 0)
                s->entry_slot = -1;
        // one-rank frames of at least kEntryMinUnits units only: a smaller
        // frame, and a rank's share of a multi-rank frame, keep the waves' own
        // prologue (both measured slower with the pre-pass)
        if (VRT_BEAM_ENTRY && slot >= 0 && render_kind(p, instrumented) == kRenderPersistFast &&
            p.tiles_this_rank > 0 && p.nranks == 1 &&
            ((int64_t)p.tiles_this_rank * 4 >= kEntryMinUnits || (p.test_flags & VRT_TEST_SMALL_BEAM_ENTRY))) {
                // the slot's record buffer, sized for this rank's units; one
                // that must grow has no work in flight left after the host's
                // wait for the slot's last launch
                const int64_t nu = (int64_t)p.tiles_this_rank * 4;
                const size_t need = (size_t)nu * kEntryWords * sizeof(uint32_t);
                DevMem &d = s->d_entry[slot];
                if (d.size() < need) {
                        e = s->q_use[slot].sync();
                        if (e == hipSuccess)
                                e = d.alloc(need);
                }
                entry = d.as<uint32_t>();
                s->entry_slot = e == hipSuccess ? slot : -1;
                s->entry_units = nu;
        }
        if (e == hipSuccess)
                e = launch_render(p, instrumented, st, &waves, units, s->ord_wmin, entry);
        if (e != hipSuccess) {
                if (slot >= 0)
                        queue_reset(s, slot, st);
                return fail(VRT_E_DEVICE, "render launch failed: %s", hipGetErrorString(e));
        }
        if (slot >= 0)
                return queue_release(s, slot, st, units, waves);
        return VRT_OK;
}

static int ts_acquire(vrt_scene *s, int i, hipStream_t st);
static int ts_release(vrt_scene *s, int i, hipStream_t st);

// Compaction queue of one config-5 launch (SpillQueues).  Its
// size is an estimate: when the queue is full, the rays that stop finish
// their walks in place (spill_room), so any size gives the same images.  The
// first launch sizes queue 0 for 1/32 of the rank's secondary rays (1080p:
// 4.1 M 64-B records, 0.26 GB) plus one partly filled chunk per resident
// wave; after every launch its counters are copied to pinned memory, and a
// later launch sizes for 1.25 x the records its phase A stopped (queued +
// finished in place), growing, never shrinking, and never past 1 GiB per set.
// Only queue 0's records are allocated: the one pooled resume round walks
// every saved ray to its end (queue 1's fill words list the streaming round's
// leftover chunks).  The scene keeps two sets; a stream keeps using the set
// it used last (stream order protects it), an idle set is shared, and a
// second set is allocated only for frames in flight on two streams (the new
// stream waits for the set's last user's event).  sq->nchunks stays 0 (no
// compaction) when the build disables it, the film has 2^26 pixels or more,
// the octree 2^24 nodes or more (SpillRec's packed words), or the allocation
// fails.
// chunks: the records, their two fill words, the counters and the deferred-
// pixel list (dpb bytes) within 1 GiB
static uint32_t spill_cap_max(size_t dpb)
{
        return (uint32_t)((((size_t)1 << 30) - 4096 - dpb) / ((size_t)kSpillChunk * sizeof(SpillRec) + 8));
}
static size_t spill_dpix_bytes(int64_t pixels)
{
        return ((size_t)pixels * 4 + 255) & ~(size_t)255;
}
static size_t spill_set_bytes(uint32_t nch, int64_t pixels)
{
        const size_t fb = ((size_t)nch * 4 + 255) & ~(size_t)255;
        return (size_t)kSpillMaxRounds * kSpillCtrStride * 4 + 2 * fb + (size_t)nch * kSpillChunk * sizeof(SpillRec) +
               spill_dpix_bytes(pixels);
}
static int spill_setup(vrt_scene *s, int64_t rays, int64_t pixels, hipStream_t st, SpillQueues *sq, int *set)
{
        *sq = spill_defaults();
        *set = -1;
        // SpillRec packs the pixel in 26 bits and a stack entry's block in 24
        if (sq->t_first == 0 || rays <= 0 || pixels >= (int64_t)1 << 26 || s->nodes.size() >= ((size_t)1 << 24))
                return VRT_OK;
        // this stream's own set; else an allocated set whose last launch has
        // finished (a second set is allocated only for frames in flight on
        // two streams); else the next one
        int k = -1;
        for (int i = 0; i < 2 && k < 0; ++i)
                if (s->spill_use[i].live && s->spill_stream[i] == st)
                        k = i;
        for (int i = 0; i < 2 && k < 0; ++i)
                if (s->d_spill[i] && s->spill_use[i].done())
                        k = i;
        if (k < 0) {
                k = s->spill_next;
                s->spill_next ^= 1;
        }
        LastUse &use = s->spill_use[k];
        if (!use.ev)
                HIPCHK(use.create());
        if (!s->spill_side[k].st) {
                // all three or none (a set without a side stream runs the
                // deferred walk on the launch's stream)
                SideStream sl;
                if (sl.fork.create(hipEventDisableTiming) == hipSuccess &&
                    sl.join.create(hipEventDisableTiming) == hipSuccess && sl.st.create() == hipSuccess)
                        s->spill_side[k] = std::move(sl);
                else
                        (void)hipGetLastError();
        }
        if (!s->h_spill) {
                HIPCHK(s->h_spill.alloc(16 * sizeof(uint32_t)));
                std::memset(s->h_spill, 0, 16 * sizeof(uint32_t));
        }
        const uint32_t *h_ctr = s->h_spill.as<uint32_t>();
        // the deferred-pixel list holds one entry per pixel of the film
        const int64_t px = std::max<int64_t>(pixels, s->spill_px[k]);
        const uint32_t cap_max = spill_cap_max(spill_dpix_bytes(px));
        // what the finished launches of either set stopped: records queued
        // (ctr[2]) + records finished in place for want of room (ctr[5])
        for (int i = 0; i < 2; ++i)
                if (s->spill_use[i].live && s->spill_cap[i] && s->spill_use[i].done()) {
                        const uint64_t need = (uint64_t)h_ctr[8 * i + 2] + h_ctr[8 * i + 5];
                        const uint64_t w = (need * 5 / 4 + kSpillChunk - 1) / kSpillChunk;
                        s->spill_want = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(s->spill_want, w), cap_max);
                }
        if (s->spill_stream[k] != st)
                HIPCHK(use.wait(st));
        // + one partly filled chunk per wave of a resident grid
        const int64_t partial = (int64_t)std::max(1, s->dev.sec_blocks) * 4;
        const int64_t est = s->spill_want ? (int64_t)s->spill_want : (rays / 32 + kSpillChunk - 1) / kSpillChunk;
        const uint32_t nch = (uint32_t)std::min<int64_t>(std::min<int64_t>(est, (rays + kSpillChunk - 1) / kSpillChunk) +
                                                                 partial, cap_max);
        const size_t ctr_bytes = (size_t)kSpillMaxRounds * kSpillCtrStride * 4;
        if (s->spill_cap[k] < nch || s->spill_px[k] < pixels) {
                // a regrowth for a larger film keeps the chunks it had
                const uint32_t c = std::min(std::max(nch, s->spill_cap[k]), cap_max);
                if (s->d_spill[k]) {
                        // the set's users on any stream are ordered by its event
                        // (spill_done after each, a stream wait when a set
                        // changes stream): the last one's event covers them all
                        HIPCHK(use.sync());
                        s->d_spill[k].reset();
                        s->spill_cap[k] = 0;
                        s->spill_px[k] = 0;
                }
                if (s->d_spill[k].alloc(spill_set_bytes(c, px)) != hipSuccess) {
                        (void)hipGetLastError();
                        return VRT_OK;  // no compaction
                }
                s->spill_cap[k] = c;
                s->spill_px[k] = px;
        }
        const size_t fb = ((size_t)s->spill_cap[k] * 4 + 255) & ~(size_t)255;
        char *b = s->d_spill[k].as<char>();
        sq->ctr = reinterpret_cast<uint32_t *>(b);
        sq->fill[0] = reinterpret_cast<uint32_t *>(b + ctr_bytes);
        sq->fill[1] = reinterpret_cast<uint32_t *>(b + ctr_bytes + fb);
        sq->rec[0] = reinterpret_cast<SpillRec *>(b + ctr_bytes + 2 * fb);
        sq->rec[1] = nullptr;  // the pooled resume round stops no ray
        sq->nchunks = s->spill_cap[k];
        sq->dpix = reinterpret_cast<uint32_t *>(b + ctr_bytes + 2 * fb +
                                                (size_t)s->spill_cap[k] * kSpillChunk * sizeof(SpillRec));
        HIPCHK(hipMemsetAsync(sq->ctr, 0, ctr_bytes, st));
        *set = k;
        return VRT_OK;
}

// After a config-5 launch with compaction set k on st: its counters to
// pinned memory (spill_setup reads them once the set's event has passed) and
// the set's event.
static int spill_done(vrt_scene *s, int k, const SpillQueues &sq, hipStream_t st)
{
        HIPCHK(hipMemcpyAsync(s->h_spill.as<uint32_t>() + 8 * k, sq.ctr, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost,
                              st));
        HIPCHK(s->spill_use[k].record(st));
        s->spill_stream[k] = st;
        return VRT_OK;
}

// One config-5 launch (k_primary1 + secondary rays) on stream st (caller
// holds s->mu).  share: the share-sized primary pass (PrimShare) instead of
// the whole-film one.
static int secondary_launch(vrt_scene *s, const RenderParams &p, int spp, int rank, int nranks, float *d_prim,
                            float *d_vis, int32_t *s_hit, int32_t *s_tri, uint32_t *s_vox, hipStream_t st,
                            const PrimShare *share = nullptr)
{
        int slot = -1;
        WorkQueue q;
        std::memset(&q, 0, sizeof q);
        (void)hipGetLastError();  // a leftover error of an earlier call is not this launch's
        SpillQueues sq;
        std::memset(&sq, 0, sizeof sq);
        int set = -1;
        if (secondary_uses_queue(p.sc)) {
                if (int rc = queue_take(s, st, &q, &slot))
                        return rc;
                if (!s_tri && !s_vox) {  // the occlusion walk: compaction
                        const int64_t rays = deal_count(tile_deal(p.ntx, p.nty, nranks), rank) * 64 * (int64_t)spp;
                        if (int rc = spill_setup(s, rays, (int64_t)p.ntx * 8 * p.nty * 8, st, &sq, &set))
                                return rc;
                }
        }
        int waves = 0, units[8];
        s->spill_last = sq.nchunks > 0 ? set : -1;
        SideLaunch side{};
        if (set >= 0)
                side = { s->spill_side[set].st, s->spill_side[set].fork, s->spill_side[set].join };
        const hipError_t e = launch_secondary(p, spp, rank, nranks, scene_res(s), d_prim, d_vis, s_hit, s_tri,
                                              s_vox, slot >= 0 ? &q : nullptr, st, &waves, units, &sq,
                                              side.st ? &side : nullptr, share);
        if (set >= 0)
                if (int rc = spill_done(s, set, sq, st))
                        return rc;
        if (e != hipSuccess) {
                if (slot >= 0)
                        queue_reset(s, slot, st);
                return fail(VRT_E_DEVICE, "secondary launch failed: %s", hipGetErrorString(e));
        }
        if (slot >= 0)
                return queue_release(s, slot, st, units, waves);
        return VRT_OK;
}

// A trace scratch set (vrt_scene::ts) serves one user at a time: the next
// user's stream waits for the previous user's (caller holds s->mu).
static int ts_acquire(vrt_scene *s, int i, hipStream_t st)
{
        HIPCHK(s->ts[i].use.wait(st));
        return VRT_OK;
}

static int ts_release(vrt_scene *s, int i, hipStream_t st)
{
        HIPCHK(s->ts[i].use.record(st));
        return VRT_OK;
}

// set i's light-map block (nodes x (LMRec + float4) + the flag word)
// Per node, the cell a cone march's descent to it implies (TraceParams::
// cells): the root's is all of space; a child's is its parent's cut at the
// parent's box centre (AABB3D::center, as k_lm_aux computes it) on the side
// of the child's octant -- per axis the tightest (lo, hi] the descent's
// `pt > centre` choices establish.
static std::vector<float4> cone_cells(const std::vector<NodeRec> &nodes)
{
        const float inf = std::numeric_limits<float>::infinity();
        std::vector<float4> c(2 * nodes.size());
        if (nodes.empty())
                return c;
        c[0] = make_float4(-inf, -inf, -inf, 0.f);
        c[1] = make_float4(inf, inf, inf, 0.f);
        for (size_t i = 0; i < nodes.size(); ++i) {  // BFS order: parents first
                const NodeRec &nr = nodes[i];
                if (nr.a & kLeafBit)
                        continue;
                const float cx = (nr.bmin[0] + nr.bmax[0]) * .5f, cy = (nr.bmin[1] + nr.bmax[1]) * .5f,
                            cz = (nr.bmin[2] + nr.bmax[2]) * .5f;
                for (uint32_t o = 0; o < 8; ++o) {
                        float4 lo = c[2 * i], hi = c[2 * i + 1];
                        if (o & 4) lo.x = std::max(lo.x, cx); else hi.x = std::min(hi.x, cx);
                        if (o & 2) lo.y = std::max(lo.y, cy); else hi.y = std::min(hi.y, cy);
                        if (o & 1) lo.z = std::max(lo.z, cz); else hi.z = std::min(hi.z, cz);
                        c[2 * (size_t)(nr.a + o)] = lo;
                        c[2 * (size_t)(nr.a + o) + 1] = hi;
                }
        }
        return c;
}

// Trace set i's block: light map, cone-descent records, finiteness flag
// (256 B), then the nodes' cone cells (static, filled on allocation).
// One trace set's light-map block: the light map (LMRec per node), the
// cone-descent records (float4 per node), the non-finite flag (256 B) and the
// per-node cells (2 float4 per node)
static size_t lm_set_bytes(size_t n)
{
        return n * (sizeof(LMRec) + sizeof(float4)) + 256 + n * 2 * sizeof(float4);
}

static int ensure_lm(vrt_scene *s, int i)
{
        if (!s->ts[i].lm) {
                const size_t n = s->nodes.size();
                HIPCHK(s->ts[i].lm.alloc(lm_set_bytes(n)));
                const std::vector<float4> cells = cone_cells(s->nodes);
                HIPCHK(hipMemcpy(s->ts[i].lm.as<char>() + n * (sizeof(LMRec) + sizeof(float4)) + 256,
                                 cells.data(), cells.size() * sizeof(float4), hipMemcpyHostToDevice));
        }
        return VRT_OK;
}

// The rank's tabled deal (RenderParams::tile_xy) for nranks > 1, built on
// first use on stream st; a stream other than the builder's waits for the
// build.  nullptr (the kernels then compute the deal): one rank, tile grids
// of 2^16 or more, more than kDealMaps deals in use, or no memory.
constexpr size_t kDealMaps = 32;
static const uint32_t *deal_map(vrt_scene *s, int ntx, int nty, int nranks, int rank, hipStream_t st)
{
        if (nranks <= 1 || ntx >= 65536 || nty >= 65536)
                return nullptr;
        for (auto &m : s->dmaps)
                if (m.ntx == ntx && m.nty == nty && m.nranks == nranks && m.rank == rank) {
                        if (!m.built.done() && m.built.wait(st) != hipSuccess) {
                                (void)hipGetLastError();
                                return nullptr;
                        }
                        return m.d.as<uint32_t>();
                }
        const int n = deal_count(tile_deal(ntx, nty, nranks), rank);
        if (n <= 0 || s->dmaps.size() >= kDealMaps)
                return nullptr;
        try {
                s->dmaps.reserve(kDealMaps);  // the push_back below cannot fail
        } catch (const std::bad_alloc &) {
                return nullptr;
        }
        vrt_scene::DealMap m{ ntx, nty, nranks, rank, {}, {} };
        if (m.d.alloc((size_t)n * sizeof(uint32_t)) != hipSuccess || m.built.create() != hipSuccess ||
            launch_deal_map(ntx, nty, nranks, rank, m.d.as<uint32_t>(), st) != hipSuccess ||
            m.built.record(st) != hipSuccess) {
                (void)hipGetLastError();
                // a launch that got as far as the stream finishes before m frees the map
                if (m.d)
                        (void)hipStreamSynchronize(st);
                return nullptr;
        }
        s->dmaps.push_back(std::move(m));
        return s->dmaps.back().d.as<uint32_t>();
}

extern "C" int vrt_render_tiles_device(vrt_scene *s, const vrt_camera *cam,
                                       const vrt_film *film, int rank,
                                       int nranks, int image_layout,
                                       float *d_out, void *stream)
{
        if (s && need_device(s))
                return VRT_E_NODEVICE;
        if (!s || !cam || !d_out)
                return fail(VRT_E_INVALID, "null argument");
        if (int rc = film_ok(film))
                return rc;
        if (nranks < 1 || rank < 0 || rank >= nranks)
                return fail(VRT_E_INVALID, "rank %d of %d", rank, nranks);
        if (image_layout && nranks != 1)
                return fail(VRT_E_INVALID, "image_layout requires nranks == 1");
        std::lock_guard<std::mutex> lk(s->mu);
        HIPCHK(hipSetDevice(s->device));
        RenderParams p;
        fill_render_params(s, cam, film, rank, nranks, &p);
        p.image_layout = image_layout;
        p.out = d_out;
        hipStream_t st = static_cast<hipStream_t>(stream);
        p.tile_xy = deal_map(s, p.ntx, p.nty, nranks, rank, st);
        HIPCHK(hipEventRecord(s->ev0, st));
        if (int rc = render_launch(s, p, false, st))
                return rc;
        HIPCHK(hipEventRecord(s->ev1, st));
        s->timed = true;
        return VRT_OK;
}

extern "C" int vrt_last_kernel_ms(vrt_scene *s, float *ms)
{
        if (!s || !ms)
                return fail(VRT_E_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(s->mu);
        if (!s->timed)
                return fail(VRT_E_INVALID, "no timed launch yet");
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(hipEventSynchronize(s->ev1));
        HIPCHK(hipEventElapsedTime(ms, s->ev0, s->ev1));
        return VRT_OK;
}

extern "C" int vrt_unpack_tiles_device(const vrt_film *film, int nranks,
                                       const float *d_gathered, float *d_image,
                                       void *stream)
{
        if (!d_gathered || !d_image || nranks < 1)
                return fail(VRT_E_INVALID, "bad argument");
        if (int rc = film_ok(film))
                return rc;
        const int tpr = vrt_tiles_per_rank(film, nranks);
        HIPCHK(launch_unpack(film->nx, film->ny, film->nx / 8, film->ny / 8, nranks, tpr,
                             d_gathered, d_image, static_cast<hipStream_t>(stream)));
        return VRT_OK;
}

extern "C" int vrt_pack_tiles_c_device(const vrt_film *film, int rank, int nranks, int comps, const float *d_image,
                                       float *d_packed, void *stream)
{
        if (!d_image || !d_packed || nranks < 1 || rank < 0 || rank >= nranks || comps < 1 || comps > 4)
                return fail(VRT_E_INVALID, "bad argument");
        if (int rc = film_ok(film))
                return rc;
        HIPCHK(launch_pack_c(film->nx, film->ny, rank, nranks, comps, d_image, d_packed,
                             static_cast<hipStream_t>(stream)));
        return VRT_OK;
}

extern "C" int vrt_unpack_tiles_c_device(const vrt_film *film, int nranks, int comps, const float *d_gathered,
                                         float *d_image, void *stream)
{
        if (!d_gathered || !d_image || nranks < 1 || comps < 1 || comps > 4)
                return fail(VRT_E_INVALID, "bad argument");
        if (int rc = film_ok(film))
                return rc;
        HIPCHK(launch_unpack_c(film->nx, film->ny, nranks, vrt_tiles_per_rank(film, nranks), comps, d_gathered,
                               d_image, static_cast<hipStream_t>(stream)));
        return VRT_OK;
}

extern "C" int vrt_rgbe_device(const float *d_img, int w, int h, int comp, uint8_t *d_rgbe, void *stream)
{
        if (!d_img || !d_rgbe || w <= 0 || h <= 0 || comp < 1 || comp > 4)
                return fail(VRT_E_INVALID, "vrt_rgbe_device: bad argument");
        HIPCHK(launch_rgbe(d_img, (int64_t)w * h, comp, d_rgbe, static_cast<hipStream_t>(stream)));
        return VRT_OK;
}

// memcpy of a large host range split over up to 4 threads (pinned staging
// <-> the caller's pageable arrays: one core's memcpy is well below PCIe)
void vrt::par_memcpy(void *dst, const void *src, size_t bytes)
{
        const int nth = bytes >= ((size_t)4 << 20) ? 4 : 1;
        if (nth == 1) {
                std::memcpy(dst, src, bytes);
                return;
        }
        auto part = [&](int j) {
                const size_t a = (bytes * j / nth) & ~(size_t)63, b = j + 1 == nth ? bytes : (bytes * (j + 1) / nth) & ~(size_t)63;
                std::memcpy(static_cast<char *>(dst) + a, static_cast<const char *>(src) + a, b - a);
        };
        std::vector<std::thread> th;
        for (int j = 1; j < nth; ++j)
                th.emplace_back(part, j);
        part(0);
        for (auto &t : th)
                t.join();
}

// vrt_render into a host array (no per-sample outputs): the device image and
// a pinned staging copy are kept in the scene; the frame is rendered as
// kOutBands tile-row bands alternating over two streams (half-chip grids, so
// a band's ramp-down runs beside the next band), each band copied D2H into
// the pinned buffer on a copy stream as soon as it is rendered, and copied
// on to `rgb` by up to 4 host threads as its copy lands.  The same kernels
// and pixels as the one-launch render (a pixel's value does not depend on
// the launch it belongs to).  Caller holds s->mu, device set.
static int render_to_host(vrt_scene *s, const vrt_camera *cam, const vrt_film *film, float *rgb)
{
        HostOut &ho = s->ho;
        const int nx = film->nx, ny = film->ny, ntx = nx / 8, nty = ny / 8;
        const size_t bytes = (size_t)nx * ny * 12;
        if (ntx == 0 || nty == 0) {  // no 8x8 tile: render_mt renders nothing
                std::memset(rgb, 0, bytes);
                return VRT_OK;
        }
        if (!ho.ev_j) {  // the last one made
                HIPCHK(ho.st2.create());
                HIPCHK(ho.cp.create());
                for (int b = 0; b < kOutBands; ++b) {
                        HIPCHK(ho.ev_r[b].create(hipEventDisableTiming));
                        HIPCHK(ho.ev_c[b].create(hipEventDisableTiming));
                }
                HIPCHK(ho.ev_j.create(hipEventDisableTiming));
        }
        if (ho.nx != nx || ho.ny != ny) {
                HIPCHK(ho.img.grow(bytes, ho.cp));  // the copy stream is the pair's last user
                // pixels outside the tile grid are never written: zero once per film shape
                HIPCHK(hipMemsetAsync(ho.img.d, 0, bytes, s->stream));
                ho.nx = nx;
                ho.ny = ny;
        }
        const int nb = std::min(kOutBands, nty);
        HIPCHK(hipEventRecord(s->ev0, s->stream));
        HIPCHK(hipEventRecord(ho.ev_j, s->stream));
        HIPCHK(hipStreamWaitEvent(ho.st2, ho.ev_j, 0));
        size_t off[kOutBands + 1];
        for (int b = 0; b < nb; ++b) {
                const int r0 = b * nty / nb, r1 = (b + 1) * nty / nb;
                hipStream_t st = (b & 1) ? ho.st2 : s->stream;
                RenderParams p;
                fill_render_params(s, cam, film, 0, 1, &p);
                p.nty = r1 - r0;
                p.ty0 = r0;
                p.tiles_this_rank = ntx * (r1 - r0);
                p.sc.grid_div = nb > 1 ? 2 : 1;
                p.image_layout = 1;
                p.out = ho.img.d.as<float>();
                if (int rc = render_launch(s, p, false, st))
                        return rc;
                HIPCHK(hipEventRecord(ho.ev_r[b], st));
                HIPCHK(hipStreamWaitEvent(ho.cp, ho.ev_r[b], 0));
                // band b's rows (the last band also carries the rows below the grid)
                off[b] = b == 0 ? 0 : (size_t)8 * r0 * nx * 12;
                off[b + 1] = b + 1 == nb ? bytes : (size_t)8 * r1 * nx * 12;
                HIPCHK(hipMemcpyAsync(ho.img.h.as<char>() + off[b], ho.img.d.as<char>() + off[b], off[b + 1] - off[b],
                                      hipMemcpyDeviceToHost, ho.cp));
                HIPCHK(hipEventRecord(ho.ev_c[b], ho.cp));
        }
        HIPCHK(hipEventRecord(ho.ev_j, ho.st2));
        HIPCHK(hipStreamWaitEvent(s->stream, ho.ev_j, 0));
        HIPCHK(hipEventRecord(s->ev1, s->stream));
        s->timed = true;
        // copy-out: band b as soon as its D2H copy has landed
        std::atomic<bool> bad{ false };
        const int nth = bytes >= ((size_t)4 << 20) ? 4 : 1;
        auto work = [&](int j) {
                for (int b = 0; b < nb; ++b) {
                        if (hipEventSynchronize(ho.ev_c[b]) != hipSuccess) {
                                bad = true;
                                return;
                        }
                        const size_t n = off[b + 1] - off[b];
                        const size_t a = off[b] + ((n * j / nth) & ~(size_t)63);
                        const size_t e = j + 1 == nth ? off[b + 1] : off[b] + ((n * (j + 1) / nth) & ~(size_t)63);
                        std::memcpy(reinterpret_cast<char *>(rgb) + a, ho.img.h.as<char>() + a, e - a);
                }
        };
        std::vector<std::thread> th;
        for (int j = 1; j < nth; ++j)
                th.emplace_back(work, j);
        work(0);
        for (auto &t : th)
                t.join();
        HIPCHK(hipStreamSynchronize(s->stream));
        if (bad)
                return fail(VRT_E_DEVICE, "vrt_render: device-to-host copy failed");
        return VRT_OK;
}

extern "C" int vrt_render(vrt_scene *s, const vrt_camera *cam,
                          const vrt_film *film, float *rgb,
                          const vrt_samples *samples, vrt_stats *stats)
{
        if (s && need_device(s))
                return VRT_E_NODEVICE;
        if (!s || !cam || !rgb)
                return fail(VRT_E_INVALID, "null argument");
        if (int rc = film_ok(film))
                return rc;
        std::lock_guard<std::mutex> lk(s->mu);
        HIPCHK(hipSetDevice(s->device));
        const bool no_samples = !samples || !(samples->hit || samples->tri || samples->voxel || samples->rgb ||
                                              samples->counters);
        if (no_samples && !stats)
                return render_to_host(s, cam, film, rgb);
        const size_t npix = (size_t)film->nx * film->ny;
        const size_t ns = npix * 4;
        const bool want_cnt = (samples && samples->counters) || stats;
        if (want_cnt)
                if (int rc = no_probe_scene(s, "vrt_render with instrumented counters"))
                        return rc;
        DevMem img, shit, stri, svox, srgb, scnt;
        HIPCHK(img.alloc(npix * 3 * sizeof(float)));
        HIPCHK(hipMemsetAsync(img, 0, npix * 3 * sizeof(float), s->stream));
        RenderParams p;
        fill_render_params(s, cam, film, 0, 1, &p);
        p.sc.grid_div = 1;  // synchronous: one frame at a time, the whole chip
        p.image_layout = 1;
        p.out = img.as<float>();
        auto alloc_fill = [&](DevMem &b, size_t bytes, int byte) -> hipError_t {
                hipError_t e = b.alloc(bytes);
                if (e != hipSuccess)
                        return e;
                return hipMemsetAsync(b, byte, bytes, s->stream);
        };
        if (samples && samples->hit) {
                HIPCHK(alloc_fill(shit, ns * 4, 0));
                p.so.hit = shit.as<int32_t>();
        }
        if (samples && samples->tri) {
                HIPCHK(alloc_fill(stri, ns * 4, 0xFF));
                p.so.tri = stri.as<int32_t>();
        }
        if (samples && samples->voxel) {
                HIPCHK(alloc_fill(svox, ns * 4, 0xFF));
                p.so.vox = svox.as<uint32_t>();
        }
        if (samples && samples->rgb) {
                HIPCHK(alloc_fill(srgb, ns * 12, 0));
                p.so.rgb = srgb.as<float>();
        }
        if (want_cnt) {
                HIPCHK(alloc_fill(scnt, ns * 16, 0));
                p.so.cnt = scnt.as<uint32_t>();
        }
        HIPCHK(hipEventRecord(s->ev0, s->stream));
        if (int rc = render_launch(s, p, want_cnt, s->stream))
                return rc;
        HIPCHK(hipEventRecord(s->ev1, s->stream));
        s->timed = true;
        HIPCHK(hipStreamSynchronize(s->stream));
        HIPCHK(hipMemcpy(rgb, img, npix * 3 * sizeof(float), hipMemcpyDeviceToHost));
        if (p.so.hit)
                HIPCHK(hipMemcpy(samples->hit, shit, ns * 4, hipMemcpyDeviceToHost));
        if (p.so.tri)
                HIPCHK(hipMemcpy(samples->tri, stri, ns * 4, hipMemcpyDeviceToHost));
        if (p.so.vox)
                HIPCHK(hipMemcpy(samples->voxel, svox, ns * 4, hipMemcpyDeviceToHost));
        if (p.so.rgb)
                HIPCHK(hipMemcpy(samples->rgb, srgb, ns * 12, hipMemcpyDeviceToHost));
        std::vector<uint32_t> cnt;
        if (want_cnt) {
                cnt.resize(ns * 4);
                HIPCHK(hipMemcpy(cnt.data(), scnt, ns * 16, hipMemcpyDeviceToHost));
                if (samples && samples->counters)
                        std::memcpy(samples->counters, cnt.data(), ns * 16);
        }
        if (stats) {
                std::memset(stats, 0, sizeof *stats);
                const int W8 = 8 * (film->nx / 8), H8 = 8 * (film->ny / 8);
                for (int py = 0; py < H8; ++py)
                        for (int px = 0; px < W8; ++px)
                                for (int q = 0; q < 4; ++q) {
                                        const uint32_t *c = &cnt[(((size_t)py * film->nx + px) * 4 + q) * 4];
                                        stats->rays++;
                                        stats->aabb_tests += c[0];
                                        stats->leaves += c[1];
                                        stats->tri_tests += c[2];
                                        stats->hits += c[3];
                                }
                float ms = 0.f;
                HIPCHK(hipEventElapsedTime(&ms, s->ev0, s->ev1));
                stats->kernel_ms = ms;
        }
        return VRT_OK;
}

// Res = *min_element(root.aabb.size() / powf(2, max_depth)) (VRT/main.cc:69-70)
static float scene_res(const vrt_scene *s)
{
        const float p2 = std::pow(2.f, (float)s->max_depth);
        float res = 0.f;
        for (int k = 0; k < 3; ++k) {
                const float v = (s->info.root_max[k] - s->info.root_min[k]) / p2;
                if (k == 0 || v < res)
                        res = v;
        }
        return res;
}

// One rank's config-5 share on st (arguments checked; takes s->mu).  share:
// nullptr = the primary pass covers every pixel, else it covers the rank's
// tiles (PrimShare).
static int secondary_share(vrt_scene *s, const vrt_camera *cam, const vrt_film *film, int spp, int rank, int nranks,
                           float *d_prim, float *d_vis, const PrimShare *share, hipStream_t st)
{
        std::lock_guard<std::mutex> lk(s->mu);
        HIPCHK(hipSetDevice(s->device));
        RenderParams p;
        fill_render_params(s, cam, film, 0, 1, &p);
        // the secondary rays' share
        p.tile_xy = deal_map(s, p.ntx, p.nty, nranks, rank, st);
        HIPCHK(hipEventRecord(s->ev0, st));
        if (int rc = secondary_launch(s, p, spp, rank, nranks, d_prim, d_vis, nullptr, nullptr, nullptr, st, share))
                return rc;
        HIPCHK(hipEventRecord(s->ev1, st));
        s->timed = true;
        return VRT_OK;
}

extern "C" int vrt_render_secondary_device(vrt_scene *s, const vrt_camera *cam,
                                           const vrt_film *film, int spp,
                                           int rank, int nranks, float *d_prim,
                                           float *d_vis, void *stream)
{
        if (s && need_device(s))
                return VRT_E_NODEVICE;
        if (!s || !cam || !d_prim || !d_vis || spp < 1 || spp > 64)
                return fail(VRT_E_INVALID, "bad argument (spp must be 1..64)");
        if (int rc = film_ok(film))
                return rc;
        if (nranks < 1 || rank < 0 || rank >= nranks)
                return fail(VRT_E_INVALID, "rank %d of %d", rank, nranks);
        // (the primary pass covers every pixel)
        return secondary_share(s, cam, film, spp, rank, nranks, d_prim, d_vis, nullptr, static_cast<hipStream_t>(stream));
}

extern "C" int vrt_render_secondary_tiles_device(vrt_scene *s, const vrt_camera *cam, const vrt_film *film, int spp,
                                                 int rank, int nranks, float *d_prim, float *d_vis, float *d_packed,
                                                 uint64_t *d_prim_hits, void *stream)
{
        if (s && need_device(s))
                return VRT_E_NODEVICE;
        if (!s || !cam || !d_prim || !d_vis || !d_packed || spp < 1 || spp > 64)
                return fail(VRT_E_INVALID, "bad argument (spp must be 1..64)");
        if (int rc = film_ok(film))
                return rc;
        if (nranks < 1 || rank < 0 || rank >= nranks)
                return fail(VRT_E_INVALID, "rank %d of %d", rank, nranks);
        hipStream_t st = static_cast<hipStream_t>(stream);
        if (d_prim_hits) {
                std::lock_guard<std::mutex> lk(s->mu);
                HIPCHK(hipSetDevice(s->device));
                HIPCHK(hipMemsetAsync(d_prim_hits, 0, sizeof(uint64_t), st));
        }
        if (deal_count(tile_deal(film->nx / 8, film->ny / 8, nranks), rank) == 0)  // no tile: nothing to render or pack
                return VRT_OK;
        const PrimShare share{ reinterpret_cast<unsigned long long *>(d_prim_hits) };
        if (int rc = secondary_share(s, cam, film, spp, rank, nranks, d_prim, d_vis, &share, st))
                return rc;
        HIPCHK(launch_pack_c(film->nx, film->ny, rank, nranks, 1, d_vis, d_packed, st));
        return VRT_OK;
}

extern "C" int vrt_scene_scratch_bytes(vrt_scene *s, int64_t *bytes, int64_t *spill_bytes)
{
        if (!s || !bytes)
                return fail(VRT_E_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(s->mu);
        int64_t sp = 0;
        for (int k = 0; k < 2; ++k)
                if (s->d_spill[k])
                        sp += (int64_t)spill_set_bytes(s->spill_cap[k], s->spill_px[k]);
        int64_t t = sp + (int64_t)s->d_light.size() + (int64_t)s->ho.img.cap + (int64_t)s->tb.cap;
        for (const TraceSet &ts : s->ts)
                t += (int64_t)(ts.lm.size() + ts.rec.size());
        for (const DevMem &e : s->d_entry)  // the beam-entry records of the ring slots used so far
                t += (int64_t)e.size();
        for (const auto &m : s->dmaps)  // the tabled multi-rank deals
                t += (int64_t)deal_count(tile_deal(m.ntx, m.nty, m.nranks), m.rank) * (int64_t)sizeof(uint32_t);
        *bytes = t;
        if (spill_bytes)
                *spill_bytes = sp;
        return VRT_OK;
}

extern "C" int vrt_secondary_spill_counts(vrt_scene *s, int64_t counts[4])
{
        if (s && need_device(s))
                return VRT_E_NODEVICE;
        if (!s || !counts)
                return fail(VRT_E_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(s->mu);
        for (int r = 0; r < 4; ++r)
                counts[r] = 0;
        if (s->spill_last < 0 || !s->d_spill[s->spill_last])
                return VRT_OK;
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(s->spill_use[s->spill_last].sync());  // the set's last launch
        std::vector<uint32_t> c((size_t)kSpillMaxRounds * kSpillCtrStride);
        HIPCHK(hipMemcpy(c.data(), s->d_spill[s->spill_last], c.size() * 4, hipMemcpyDeviceToHost));
        for (int r = 0; r < 4 && r < kSpillMaxRounds; ++r)
                counts[r] = c[(size_t)r * kSpillCtrStride + 2];  // records (spill_close)
        return VRT_OK;
}

extern "C" int vrt_debug_beam_entries(vrt_scene *s, uint32_t *out, int64_t max_units, int64_t *units)
{
        if (s && need_device(s))
                return VRT_E_NODEVICE;
        if (!s || !units || (max_units > 0 && !out) || max_units < 0)
                return fail(VRT_E_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(s->mu);
        *units = 0;
        if (s->entry_slot < 0 || !s->d_entry[s->entry_slot])
                return VRT_OK;
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(s->q_use[s->entry_slot].sync());  // the slot's last launch
        *units = s->entry_units;
        const int64_t n = std::min(max_units, s->entry_units);
        if (n > 0)
                HIPCHK(hipMemcpy(out, s->d_entry[s->entry_slot], (size_t)n * kEntryWords * sizeof(uint32_t),
                                 hipMemcpyDeviceToHost));
        return VRT_OK;
}

extern "C" int vrt_secondary_spill_stats(vrt_scene *s, int64_t stats[7])
{
        if (s && need_device(s))
                return VRT_E_NODEVICE;
        if (!s || !stats)
                return fail(VRT_E_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(s->mu);
        for (int r = 0; r < 7; ++r)
                stats[r] = 0;
        if (s->spill_last < 0 || !s->d_spill[s->spill_last])
                return VRT_OK;
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(s->spill_use[s->spill_last].sync());
        uint32_t c[8];
        HIPCHK(hipMemcpy(c, s->d_spill[s->spill_last], sizeof c, hipMemcpyDeviceToHost));
        stats[0] = c[2];                     // records queued (spill_close)
        stats[1] = c[5];                     // rays finished in place, queue full (spill_room)
        stats[2] = std::min(c[0], s->spill_cap[s->spill_last]);  // chunks taken
        stats[3] = s->spill_cap[s->spill_last];                  // chunks allocated
        stats[4] = c[3];                     // chunks left to the batch-pool launch
        stats[5] = (int64_t)sizeof(SpillRec);
        stats[6] = c[6];                     // pixels deferred to k_secondary_defer (exact walk)
        return VRT_OK;
}

extern "C" int vrt_render_secondary(vrt_scene *s, const vrt_camera *cam,
                                    const vrt_film *film, int spp, float *vis,
                                    int32_t *s_hit, int32_t *s_tri,
                                    uint32_t *s_vox, int64_t *rays)
{
        if (s && need_device(s))
                return VRT_E_NODEVICE;
        if (!s || !cam || !vis || spp < 1 || spp > 64)
                return fail(VRT_E_INVALID, "bad argument (spp must be 1..64)");
        if (int rc = film_ok(film))
                return rc;
        std::lock_guard<std::mutex> lk(s->mu);
        HIPCHK(hipSetDevice(s->device));
        const size_t npix = (size_t)film->nx * film->ny;
        const size_t ns = npix * (size_t)spp;
        const size_t narea = (size_t)(8 * (film->nx / 8)) * (8 * (film->ny / 8));
        DevMem dvis, dprim, dh, dt, dv;
        HIPCHK(dvis.alloc(npix * 4));
        HIPCHK(hipMemsetAsync(dvis, 0, npix * 4, s->stream));
        HIPCHK(dprim.alloc(std::max<size_t>(1, narea) * 32));
        if (s_hit) {
                HIPCHK(dh.alloc(ns * 4));
                HIPCHK(hipMemsetAsync(dh, 0, ns * 4, s->stream));
        }
        if (s_tri) {
                HIPCHK(dt.alloc(ns * 4));
                HIPCHK(hipMemsetAsync(dt, 0xFF, ns * 4, s->stream));
        }
        if (s_vox) {
                HIPCHK(dv.alloc(ns * 4));
                HIPCHK(hipMemsetAsync(dv, 0xFF, ns * 4, s->stream));
        }
        RenderParams p;
        fill_render_params(s, cam, film, 0, 1, &p);
        HIPCHK(hipEventRecord(s->ev0, s->stream));
        if (int rc = secondary_launch(s, p, spp, 0, 1, dprim.as<float>(), dvis.as<float>(),
                                      dh.as<int32_t>(), dt.as<int32_t>(),
                                      dv.as<uint32_t>(), s->stream))
                return rc;
        HIPCHK(hipEventRecord(s->ev1, s->stream));
        s->timed = true;
        HIPCHK(hipStreamSynchronize(s->stream));
        HIPCHK(hipMemcpy(vis, dvis, npix * 4, hipMemcpyDeviceToHost));
        if (s_hit)
                HIPCHK(hipMemcpy(s_hit, dh, ns * 4, hipMemcpyDeviceToHost));
        if (s_tri)
                HIPCHK(hipMemcpy(s_tri, dt, ns * 4, hipMemcpyDeviceToHost));
        if (s_vox)
                HIPCHK(hipMemcpy(s_vox, dv, ns * 4, hipMemcpyDeviceToHost));
        if (rays) {
                std::vector<float> prim(narea * 8);
                if (narea)
                        HIPCHK(hipMemcpy(prim.data(), dprim, narea * 32, hipMemcpyDeviceToHost));
                int64_t hits = 0;
                for (size_t i = 0; i < narea; ++i)
                        hits += prim[8 * i] != 0.f;
                *rays = (int64_t)narea + hits * spp;
        }
        return VRT_OK;
}

// ---------------------------------------------------------------------------
// full trace(): light map, filter, cone-tracing render
// ---------------------------------------------------------------------------
// (int)log2f(x) thresholds of the host libm: split_up[e] = smallest float in
// [2^e, 2^(e+1)) whose log2f rounds up to e+1 (+inf if none).  The cone
// march (VRT/voxel_octree.cc:286) truncates log2f; the device evaluates the
// same integer from x's exponent and this table.
static const float *split_table()
{
        static float tab[64];
        static std::once_flag once;
        std::call_once(once, [] {
                for (int e = 0; e < 64; ++e) {
                        const float lo = std::ldexp(1.0f, e), top = std::ldexp(1.0f, e + 1);
                        float t = INFINITY;
                        for (float x = std::nextafter(top, 0.0f); x >= lo; x = std::nextafter(x, 0.0f)) {
                                volatile float xv = x;
                                if ((int)log2f(xv) != e + 1)
                                        break;
                                t = x;
                        }
                        tab[e] = t;
                }
        });
        return tab;
}

extern "C" int vrt_scene_min_voxel(const vrt_scene *s, int levels, float *res)
{
        if (!s || !res)
                return fail(VRT_E_INVALID, "null argument");
        const float p2 = std::pow(2.f, (float)(levels > 0 ? levels : s->max_depth));
        for (int k = 0; k < 3; ++k) {
                const float v = (s->info.root_max[k] - s->info.root_min[k]) / p2;
                if (k == 0 || v < *res)
                        *res = v;
        }
        return VRT_OK;
}

static hipError_t ensure_light_scratch(vrt_scene *s, size_t bytes)
{
        if (s->d_light.size() >= bytes)
                return hipSuccess;
        if (s->d_light)  // used on the scene's stream only
                if (hipError_t e = hipStreamSynchronize(s->stream))
                        return e;
        return s->d_light.alloc(bytes);
}

// One light-map build between its three steps: where its lists and counters
// lie in the scene's light scratch, and what the host read at the sync.
struct LightBuild {
        int set = 0, kbits = 1, lbits = 1;
        int64_t ns = 0;        // samples of the whole light film (what the scratch holds)
        int64_t ns_rank = 0;   // samples this rank marches
        size_t sort_bytes = 0;
        int64_t max_seg = 1;
        uint64_t *k_in = nullptr, *k_out = nullptr;
        uint32_t *v_in = nullptr, *v_out = nullptr;
        float *samp = nullptr;
        void *temp = nullptr;
        unsigned int *d_count = nullptr, *d_nseg = nullptr, *d_tail_n = nullptr;
        uint32_t *d_seg = nullptr, *d_seg_end = nullptr;
        LMRec *d_lm = nullptr;
        float4 *d_cc = nullptr;
        uint32_t *d_bad = nullptr;
        unsigned int nhit = 0;  // this rank's hits (light_wait)
};

// The light pass + filter of VRT/main.cc:75-100 on the scene's stream in
// three steps (caller holds s->mu).  Step 1: the leaf case of the filter and
// the light march of rank `rank` of `nranks` of the light film's tile deal
// (0 of 1: the whole film) into the compact hit lists.
static int light_begin(vrt_scene *s, int set, const vrt_light *lights, int nlights, bool fused, int rank, int nranks,
                       LightBuild *b)
{
        const int64_t nnodes = (int64_t)s->nodes.size();
        // fused: the *_lights calls' march over all lights (k_light_lights);
        // otherwise the one light the older calls have (k_light)
        int64_t ns = 0;
        for (int l = 0; l < nlights; ++l)
                ns += (int64_t)64 * (lights[l].film.nx / 8) * (lights[l].film.ny / 8) * 4;
        if (ns > 0x7FFFFFFF)
                return fail(VRT_E_INVALID, "light film%s too large (%lld samples)", fused ? "s" : "", (long long)ns);
        // one block: light map, cone-descent records, finiteness flag
        if (int rc = ensure_lm(s, set))
                return rc;
        b->set = set;
        b->ns = ns;
        b->d_lm = s->ts[set].lm.as<LMRec>();
        b->d_cc = reinterpret_cast<float4 *>(b->d_lm + nnodes);
        b->d_bad = reinterpret_cast<uint32_t *>(b->d_cc + nnodes);
        if (int rc = ts_acquire(s, set, s->stream))  // a trace render may still read this set
                return rc;
        // scratch (sized for every sample hitting): 64-bit keys and 32-bit
        // slots in + out, the per-hit (illum, normal) records and their copy
        // in sorted order, the sort's temp, the counters, the leaf runs
        size_t sort_bytes = 0;
        int kbits = 1, lbits = 1;
        while (kbits < 40 && (ns - 1) >> kbits)
                ++kbits;
        while (lbits < 32 && ((uint64_t)nnodes >> lbits) != 0)
                ++lbits;
        HIPCHK(sort_pairs_u64(nullptr, &sort_bytes, nullptr, nullptr, nullptr, nullptr, ns, kbits + lbits, s->stream));
        const size_t b4 = align_up((size_t)ns * 4), b8 = align_up((size_t)ns * 8), b24 = align_up((size_t)ns * 48);
        b->max_seg = std::max<int64_t>(1, s->info.nonempty_leaves);
        const size_t bseg = align_up((size_t)b->max_seg * 4);
        const size_t bend = align_up((size_t)nnodes * 4);
        const size_t need = 2 * b8 + 2 * b4 + b24 + align_up(sort_bytes) + 256 + bseg + bend;
        HIPCHK(ensure_light_scratch(s, need));
        char *base = s->d_light.as<char>();
        b->kbits = kbits;
        b->lbits = lbits;
        b->sort_bytes = sort_bytes;
        b->k_in = reinterpret_cast<uint64_t *>(base);
        b->k_out = reinterpret_cast<uint64_t *>(base + b8);
        b->v_in = reinterpret_cast<uint32_t *>(base + 2 * b8);
        b->v_out = reinterpret_cast<uint32_t *>(base + 2 * b8 + b4);
        b->samp = reinterpret_cast<float *>(base + 2 * b8 + 2 * b4);
        b->temp = base + 2 * b8 + 2 * b4 + b24;
        char *ctr = base + 2 * b8 + 2 * b4 + b24 + align_up(sort_bytes);
        b->d_count = reinterpret_cast<unsigned int *>(ctr);
        b->d_nseg = reinterpret_cast<unsigned int *>(ctr + 64);
        b->d_tail_n = reinterpret_cast<unsigned int *>(ctr + 128);
        b->d_seg = reinterpret_cast<uint32_t *>(ctr + 256);
        b->d_seg_end = reinterpret_cast<uint32_t *>(ctr + 256 + bseg);
        LightParams lp;
        std::memset(&lp, 0, sizeof lp);
        fill_render_params(s, &lights[0].cam, &lights[0].film, rank, nranks, &lp.r);
        LightsParams lq;
        if (fused) {
                std::memset(&lq, 0, sizeof lq);
                lq.nlights = nlights;
                int64_t units = 0, base = 0;
                for (int l = 0; l < VRT_MAX_LIGHTS; ++l) {
                        if (l >= nlights) {
                                lq.unit_end[l] = INT32_MAX;
                                continue;
                        }
                        RenderParams rp;
                        fill_render_params(s, &lights[l].cam, &lights[l].film, rank, nranks, &rp);
                        LightEntry &e = lq.e[l];
                        e.cam = rp.cam;
                        e.ptx = rp.ntx;
                        e.pty = rp.nty;
                        e.unit_begin = (int32_t)units;
                        e.tile_xy = deal_map(s, rp.ntx, rp.nty, nranks, rank, s->stream);  // null for one rank
                        e.ntx_magic = rp.ntx_magic;
                        e.key_base = (uint64_t)base;
                        std::memcpy(e.color, lights[l].color, sizeof e.color);
                        units += (int64_t)rp.tiles_this_rank * 4;
                        base += (int64_t)64 * rp.ntx * rp.nty * 4;
                        lq.unit_end[l] = (int32_t)units;
                }
                lq.units = (int32_t)units;
                b->ns_rank = units * 64;
        } else {
                const int ptx = lights[0].film.nx / 8, pty = lights[0].film.ny / 8;
                lp.r.tile_xy = deal_map(s, ptx, pty, nranks, rank, s->stream);  // null for one rank
                b->ns_rank = (int64_t)lp.r.tiles_this_rank * 256;
                lp.ptx = ptx;
                lp.pty = pty;
        }
        lp.kbits = kbits;
        lp.count = b->d_count;
        lp.keys = b->k_in;
        lp.vals = b->v_in;
        lp.samp = b->samp;
        lp.tail_n = b->d_tail_n;
        lp.tail = b->v_out;  // free until the sort
        HIPCHK(hipEventRecord(s->ev0, s->stream));
        // cone_trace_init_filter's leaf case first: it also zeroes the
        // counters the passes below add to (no memsets)
        HIPCHK(launch_lm_leaves(s->dev.nodes, nnodes, b->d_lm, b->d_bad, b->d_count, b->d_tail_n, b->d_nseg, s->stream));
        // a leaf whose list holds probes only is non-empty too: coverage 1
        if (!s->probes.empty())
                HIPCHK(launch_lm_probe_leaves(s->dev.nodes, s->pdev.pnode, nnodes, b->d_lm, s->stream));
        if (fused) {
                lq.p = lp;
                HIPCHK(launch_light_lights(lq, s->stream));
        } else {
                HIPCHK(launch_light(lp, s->stream));
        }
        return VRT_OK;
}

// Step 2: the sort takes its length on the host, the one mid-build sync (the
// same copy reaches to the tail's sample count, final once k_light has run:
// for vrt_lightmap_stats).
static int light_wait(vrt_scene *s, LightBuild *b)
{
        unsigned int ctrs[33] = {};  // d_count at word 0, d_tail_n at word 32
        HIPCHK(hipMemcpyAsync(ctrs, b->d_count, sizeof ctrs, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
        const unsigned int nhit = ctrs[0], ntail = ctrs[32];
        b->nhit = nhit;
        s->lm_stats[0] = b->ns_rank;
        s->lm_stats[1] = nhit;
        s->lm_stats[2] = ntail;
#ifdef VRT_LIGHT_DIAG
        {
                static int ndump = 0;
                const size_t nw = (size_t)std::min<int64_t>(b->ns / 64, 1 << 20);
                std::vector<uint32_t> d(nw * 8);
                HIPCHK(light_diag_copy(d.data(), d.size() * 4));
                char name[64];
                std::snprintf(name, sizeof name, "gpurun_out/light_diag_%d.bin", ndump++);
                if (FILE *f = std::fopen(name, "wb")) {
                        std::fwrite(d.data(), 4, d.size(), f);
                        std::fclose(f);
                }
        }
#endif
#ifdef VRT_LIGHT_TAIL_REPORT
        std::fprintf(stderr, "light pass: %u of %lld samples deferred, %u hits\n", ntail, (long long)b->ns_rank, nhit);
#endif
        return VRT_OK;
}

// Step 3: sort the `total` hits of the lists (merged: the ranks' lists were
// exchanged into them, so the slots are renumbered first), the per-leaf sums
// in canonical order, the filter's internal levels; *lm_done (if given) is
// recorded after it.
static int light_finish(vrt_scene *s, LightBuild *b, unsigned int total, bool merged, hipEvent_t lm_done)
{
        const int64_t nnodes = (int64_t)s->nodes.size();
        if (merged)
                HIPCHK(launch_lm_slots(b->v_in, total, s->stream));
        if (total > 0)
                HIPCHK(sort_pairs_u64(b->temp, &b->sort_bytes, b->k_in, b->k_out, b->v_in, b->v_out, total,
                                      b->kbits + b->lbits, s->stream));
        HIPCHK(launch_lm_accum(total, b->k_out, b->v_out, b->kbits, b->samp, b->d_seg, b->d_nseg, b->max_seg,
                               b->d_seg_end, b->d_lm, s->stream));
        // cone_trace_init_filter: internal levels bottom-up
        const int nlev = (int)s->level_begin.size() - 1;
        for (int l = nlev; l >= 1; --l)
                HIPCHK(launch_lm_level(s->dev.nodes, s->level_begin[l - 1], s->level_begin[l], b->d_lm, s->stream));
        HIPCHK(launch_lm_aux(s->dev.nodes, b->d_lm, nnodes, b->d_cc, b->d_bad, s->stream));
        HIPCHK(hipEventRecord(s->ev1, s->stream));
        if (lm_done)
                HIPCHK(hipEventRecord(lm_done, s->stream));
        s->timed = true;
        s->lm_cur = b->set;
        return VRT_OK;
}

// The three steps in one call.  `overlap` (may be empty) is called right after
// the light pass is enqueued, before the mid-build host sync, so work it
// enqueues on another stream runs beside the light pass; on return the filter
// is enqueued and *lm_done (if given) recorded after it.
static int lightmap_enqueue(vrt_scene *s, int set, const vrt_light *lights, int nlights, bool fused,
                            unsigned int *hits, const std::function<int()> &overlap, hipEvent_t lm_done)
{
        LightBuild b;
        if (int rc = light_begin(s, set, lights, nlights, fused, 0, 1, &b))
                return rc;
        if (overlap)
                if (int rc = overlap())
                        return rc;
        if (int rc = light_wait(s, &b))
                return rc;
        if (int rc = light_finish(s, &b, b.nhit, false, lm_done))
                return rc;
        *hits = b.nhit;
        return VRT_OK;
}

// the one light of the calls that take a light camera and film: white, as
// the reference's driver passes it (VRT/main.cc:89-90)
static vrt_light white_light(const vrt_camera *cam, const vrt_film *film)
{
        vrt_light l;
        l.cam = *cam;
        l.film = *film;
        l.color[0] = l.color[1] = l.color[2] = 1.f;
        return l;
}

int vrt::lights_ok(const vrt_light *lights, int nlights)
{
        if (!lights)
                return fail(VRT_E_INVALID, "null argument");
        if (nlights < 1 || nlights > VRT_MAX_LIGHTS)
                return fail(VRT_E_INVALID, "nlights %d outside 1..%d", nlights, VRT_MAX_LIGHTS);
        int64_t ns = 0;
        for (int l = 0; l < nlights; ++l) {
                if (int rc = film_ok(&lights[l].film))
                        return rc;
                ns += (int64_t)64 * (lights[l].film.nx / 8) * (lights[l].film.ny / 8) * 4;
        }
        if (ns > 0x7FFFFFFF)
                return fail(VRT_E_INVALID, "light films too large (%lld samples over %d lights)", (long long)ns, nlights);
        return VRT_OK;
}

// the blocking light-map build of vrt_lightmap_build[_lights]
static int lightmap_build(vrt_scene *s, const vrt_light *lights, int nlights, bool fused, int64_t *hits)
{
        std::lock_guard<std::mutex> lk(s->mu);
        HIPCHK(hipSetDevice(s->device));
        unsigned int nhit = 0;
        const int set = s->ts_next;
        s->ts_next ^= 1;
        if (int rc = lightmap_enqueue(s, set, lights, nlights, fused, &nhit, {}, nullptr))
                return rc;
        if (int rc = ts_release(s, set, s->stream))
                return rc;
        HIPCHK(hipStreamSynchronize(s->stream));
        if (hits)
                *hits = (int64_t)nhit;
        return VRT_OK;
}

extern "C" int vrt_lightmap_build(vrt_scene *s, const vrt_camera *light_cam,
                                  const vrt_film *light_film, int64_t *hits)
{
        if (s && need_device(s))
                return VRT_E_NODEVICE;
        if (!s || !light_cam)
                return fail(VRT_E_INVALID, "null argument");
        if (int rc = film_ok(light_film))
                return rc;
        const vrt_light one = white_light(light_cam, light_film);
        return lightmap_build(s, &one, 1, false, hits);
}

extern "C" int vrt_lightmap_build_lights(vrt_scene *s, const vrt_light *lights, int nlights, int64_t *hits)
{
        if (s && need_device(s))
                return VRT_E_NODEVICE;
        if (!s)
                return fail(VRT_E_INVALID, "null argument");
        if (int rc = lights_ok(lights, nlights))
                return rc;
        return lightmap_build(s, lights, nlights, true, hits);
}

extern "C" int vrt_lightmap_stats(vrt_scene *s, int64_t stats[3])
{
        if (s && need_device(s))
                return VRT_E_NODEVICE;
        if (!s || !stats)
                return fail(VRT_E_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(s->mu);
        for (int r = 0; r < 3; ++r)
                stats[r] = s->lm_stats[r];  // read at the build's own sync
        return VRT_OK;
}

extern "C" int vrt_lightmap_nodes(vrt_scene *s, uint64_t *key, float *coverage, float *illum)
{
        if (s && need_device(s))
                return VRT_E_NODEVICE;
        if (!s || !key)
                return fail(VRT_E_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(s->mu);
        if (s->lm_cur < 0)
                return fail(VRT_E_INVALID, "no light map: call vrt_lightmap_build first");
        HIPCHK(hipSetDevice(s->device));
        const size_t n = s->nodes.size();
        std::vector<LMRec> lm(n);
        // the set may be filled on the scene stream and read on callers'
        // streams (trace frames): its last user's event covers both
        HIPCHK(hipStreamSynchronize(s->stream));
        HIPCHK(s->ts[s->lm_cur].use.sync());
        HIPCHK(hipMemcpy(lm.data(), s->ts[s->lm_cur].lm, n * sizeof(LMRec), hipMemcpyDeviceToHost));
        for (size_t l = 0; l + 1 < s->level_begin.size(); ++l)
                for (int64_t i = s->level_begin[l]; i < s->level_begin[l + 1]; ++i) {
                        key[i] = ((uint64_t)(l + 1) << 32) | s->node_vox[(size_t)i];
                        if (coverage)
                                coverage[i] = lm[(size_t)i].cov;
                        if (illum)
                                std::memcpy(illum + 18 * (size_t)i, lm[(size_t)i].illum, 18 * sizeof(float));
                }
        return VRT_OK;
}

static int trace_ok(vrt_scene *s, float min_voxel)
{
        if (!(min_voxel > 0.f))
                vrt_scene_min_voxel(s, 0, &min_voxel);
        const float mindist = 1.414f * min_voxel;
        if (!(mindist > 0.f) || !std::isfinite(mindist))
                return fail(VRT_E_INVALID, "degenerate cone step: min voxel %g (flat scene?)", (double)min_voxel);
        for (int k = 0; k < 3; ++k)
                if (!std::isfinite(s->info.root_max[k] - s->info.root_min[k]))
                        return fail(VRT_E_INVALID, "scene bounds not finite");
        return VRT_OK;
}

// nslots records: a frame's tiles_this_rank * 256 samples, or one chunk of a
// batched trace (the set serves one user at a time, so they share the block)
static int trace_scratch_n(vrt_scene *s, int set, const TraceParams &tp, size_t nslots, TraceParams *out)
{
        *out = tp;
        TraceSet &t = s->ts[set];
        // the cone step table and its length (at fixed offsets: the table
        // outlives calls with other tile counts), the primary pass's 64-B
        // records, its deferred-sample count (512 B) and list
        const size_t head = (size_t)kConeSteps * 16 + 256;
        const size_t need = head + nslots * 64 + 512 + nslots * 4;
        if (t.rec.size() < need) {
                // every user of the set's scratch is ordered by its event
                // (ts_acquire waits for it, ts_release records it)
                if (t.rec)
                        HIPCHK(t.use.sync());
                HIPCHK(t.rec.alloc(need));
                t.steps_key[0] = t.steps_key[1] = -1.f;
        }
        // the step table depends on mindist and maxdist only: rebuilt when
        // they change (the set's users are ordered by its event); the key is
        // committed only once k_cone_steps is enqueued (steps_commit)
        out->build_steps = !(t.steps_key[0] == tp.mindist && t.steps_key[1] == tp.maxdist);
        char *b = t.rec.as<char>();
        out->steps = reinterpret_cast<float4 *>(b);
        out->nsteps = reinterpret_cast<int *>(b + (size_t)kConeSteps * 16);
        out->rec = reinterpret_cast<float4 *>(b + head);
        out->tail_n = reinterpret_cast<unsigned int *>(b + head + nslots * 64);
        out->tail = reinterpret_cast<uint32_t *>(b + head + nslots * 64 + 512);
        return VRT_OK;
}

static int trace_scratch(vrt_scene *s, int set, const TraceParams &tp, TraceParams *out)
{
        return trace_scratch_n(s, set, tp, (size_t)tp.r.tiles_this_rank * 256, out);
}

// After launch_trace_prim returned success: the step table it was asked to
// build (k_cone_steps) is enqueued, so the set's key may say so.  Every error
// return before that leaves the key as it was, and the next call rebuilds.
static void steps_commit(vrt_scene *s, int set, const TraceParams &tp)
{
        if (!tp.build_steps || tp.r.tiles_this_rank <= 0)
                return;
        s->ts[set].steps_key[0] = tp.mindist;
        s->ts[set].steps_key[1] = tp.maxdist;
}

// The cone march's split level as a function of the diameter
// (TraceParams::split_bound): S(diam) = split_level_of(fl(maxdist / diam))
// -- the kernels' own rule on the correctly rounded quotient, which the host
// division reproduces -- is non-increasing in diam, so bound[k] = the
// largest float diam with S(diam) >= k, found by bisection over the float
// bit patterns (monotone in value for positive floats).
static int split_level_host(float x, const float *up)
{
        uint32_t u;
        std::memcpy(&u, &x, 4);
        const int e = (int)(u >> 23) - 127;
        if (e >= 63)
                return e;
        return x >= up[e] ? e + 1 : e;
}

static void split_bounds(float maxdist, const float *up, float *bound)
{
        static thread_local float last_max = -1.f;
        static thread_local float last[64];
        if (maxdist == last_max) {
                std::memcpy(bound, last, sizeof last);
                return;
        }
        bound[0] = maxdist;
        auto S = [&](uint32_t bits) {
                float d;
                std::memcpy(&d, &bits, 4);
                volatile float q = maxdist / d;  // one correctly rounded division, as on the device
                return split_level_host(q, up);
        };
        uint32_t top;
        std::memcpy(&top, &maxdist, 4);
        for (int k = 1; k < 64; ++k) {
                if (!(maxdist > 0.f) || !std::isfinite(maxdist) || S(1u) < k) {  // not even the least diameter
                        bound[k] = 0.f;
                        continue;
                }
                uint32_t lo = 1u, hi = top;  // S(lo) >= k; find the largest bits with S >= k
                while (lo < hi) {
                        const uint32_t mid = lo + (hi - lo + 1) / 2;
                        if (S(mid) >= k)
                                lo = mid;
                        else
                                hi = mid - 1;
                }
                std::memcpy(&bound[k], &lo, 4);
        }
        last_max = maxdist;
        std::memcpy(last, bound, sizeof last);
}

static void fill_trace_light(vrt_scene *s, int set, float min_voxel, TraceParams *tp);

static void fill_trace_params(vrt_scene *s, int set, const vrt_camera *cam, const vrt_film *film, float min_voxel,
                              int rank, int nranks, TraceParams *tp)
{
        std::memset(tp, 0, sizeof *tp);
        fill_render_params(s, cam, film, rank, nranks, &tp->r);
        fill_trace_light(s, set, min_voxel, tp);
}

// the cone march's part of TraceParams: the set's light map and the
// distances (no camera: the batched calls fill only this and the scene)
static void fill_trace_light(vrt_scene *s, int set, float min_voxel, TraceParams *tp)
{
        if (!(min_voxel > 0.f))
                vrt_scene_min_voxel(s, 0, &min_voxel);
        tp->lm = s->ts[set].lm.as<LMRec>();
        tp->cc = reinterpret_cast<const float4 *>(tp->lm + s->nodes.size());
        tp->lm_bad = reinterpret_cast<const uint32_t *>(tp->cc + s->nodes.size());
        tp->cells = reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(tp->lm_bad) + 256);
        // float mindist = 1.414f * min_voxel_size; maxdist = length(root.aabb.size())
        tp->mindist = 1.414f * min_voxel;
        const f3 sz = mk3(s->info.root_max[0] - s->info.root_min[0], s->info.root_max[1] - s->info.root_min[1],
                          s->info.root_max[2] - s->info.root_min[2]);
        tp->maxdist = length(sz);
        std::memcpy(tp->split_up, split_table(), sizeof tp->split_up);
        split_bounds(tp->maxdist, tp->split_up, tp->split_bound);
}

// ---- batched gi::ray_march (vrt_ray_march_batch[_ex][_device]) ------------
// flags: 0 or VRT_MARCH_EVEN_INVISIBLE, gi::ray_march's last parameter; it
// changes the march only on a probe scene, which then takes the mixed march
// (pd set).  An unknown flag is reported before anything else.
static int march_args_ok(vrt_scene *s, const void *rays, int64_t n, const void *hits, int flags, const ProbeDev **pd)
{
        if (flags & ~VRT_MARCH_EVEN_INVISIBLE)
                return fail(VRT_E_INVALID, "unknown flags %#x", flags);
        if (s && need_device(s))
                return VRT_E_NODEVICE;
        if (!s || n < 0 || (n > 0 && (!rays || !hits)))
                return fail(VRT_E_INVALID, "bad argument");
        *pd = (flags & VRT_MARCH_EVEN_INVISIBLE) && !s->probes.empty() ? &s->pdev : nullptr;
        return VRT_OK;
}

extern "C" int vrt_ray_march_batch_ex_device(vrt_scene *s, const vrt_ray *d_rays, int64_t n, int flags,
                                             vrt_hit *d_hits, void *stream)
{
        const ProbeDev *pd;
        if (int rc = march_args_ok(s, d_rays, n, d_hits, flags, &pd))
                return rc;
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(launch_ray_march(s->dev, d_rays, n, d_hits, static_cast<hipStream_t>(stream), s->ord_wmin, pd));
        return VRT_OK;
}

extern "C" int vrt_ray_march_batch_device(vrt_scene *s, const vrt_ray *d_rays, int64_t n, vrt_hit *d_hits,
                                          void *stream)
{
        return vrt_ray_march_batch_ex_device(s, d_rays, n, 0, d_hits, stream);
}

// host arrays: through the scene's device buffers and pinned staging
extern "C" int vrt_ray_march_batch_ex(vrt_scene *s, const vrt_ray *rays, int64_t n, int flags, vrt_hit *hits)
{
        static_assert(sizeof(vrt_ray) == 32, "vrt_ray layout");
        static_assert(sizeof(vrt_hit) == 36, "vrt_hit layout");
        const ProbeDev *pd;
        if (int rc = march_args_ok(s, rays, n, hits, flags, &pd))
                return rc;
        if (n == 0)
                return VRT_OK;
        std::lock_guard<std::mutex> lk(s->mu);
        HIPCHK(hipSetDevice(s->device));
        const size_t rbytes = (size_t)n * sizeof(vrt_ray), hbytes = (size_t)n * sizeof(vrt_hit);
        HIPCHK(s->rays.grow(rbytes, s->stream));
        HIPCHK(s->hits.grow(hbytes, s->stream));
        par_memcpy(s->rays.h, rays, rbytes);
        HIPCHK(hipMemcpyAsync(s->rays.d, s->rays.h, rbytes, hipMemcpyHostToDevice, s->stream));
        HIPCHK(launch_ray_march(s->dev, s->rays.d, n, s->hits.d, s->stream, s->ord_wmin, pd));
        HIPCHK(hipMemcpyAsync(s->hits.h, s->hits.d, hbytes, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
        par_memcpy(hits, s->hits.h, hbytes);
        return VRT_OK;
}

extern "C" int vrt_ray_march_batch(vrt_scene *s, const vrt_ray *rays, int64_t n, vrt_hit *hits)
{
        return vrt_ray_march_batch_ex(s, rays, n, 0, hits);
}

// ---- batched trace() / cone_trace (vrt_trace_batch, vrt_cone_trace_batch) --
// Records per chunk of vrt_trace_batch: the scratch (64 B each, in the
// light-map set's record block) is bounded by it whatever n is.
constexpr int64_t kBatchChunk = (int64_t)1 << 20;

static int64_t batch_chunk()
{
        return (g_test_flags.load() & VRT_TEST_SMALL_BATCH_CHUNK) ? 200 : kBatchChunk;
}

// The checks of the six batched calls (vrt_trace_batch, vrt_cone_trace_batch,
// vrt_probe_gather and their _device forms), in one order: a null scene or n
// < 0; n == 0 is VRT_OK whatever the scene is (*empty: nothing to do); a
// host-only scene; null pointers (ptrs: the call's are all set); the gather's
// point count (points set); the cone step; then, under the scene's lock, the
// light map.  VRT_OK and not *empty: *lk holds s->mu, a light map exists and
// the device is set.
static int batch_begin(vrt_scene *s, int64_t n, bool ptrs, const float *points, int npoints, float min_voxel,
                       std::unique_lock<std::mutex> *lk, bool *empty)
{
        *empty = n == 0;
        if (!s || n < 0)
                return fail(VRT_E_INVALID, "bad argument");
        if (n == 0)
                return VRT_OK;
        if (need_device(s))
                return VRT_E_NODEVICE;
        if (!ptrs)
                return fail(VRT_E_INVALID, "null argument");
        if (points && (npoints < 1 || npoints > kProbeMaxPoints))
                return fail(VRT_E_INVALID, "bad argument: %d points (1..%d)", npoints, kProbeMaxPoints);
        if (int rc = trace_ok(s, min_voxel))
                return rc;
        *lk = std::unique_lock<std::mutex>(s->mu);
        if (s->lm_cur < 0)
                return fail(VRT_E_INVALID, "no light map: call vrt_lightmap_build first");
        HIPCHK(hipSetDevice(s->device));
        return VRT_OK;
}

// One launch on stream st over the current trace set (caller holds s->mu,
// the device is set, a light map exists): the set's light map and step table
// and `nslots` records of its block behind the first rec_skip, taken and
// released through the set's event like a frame -- after a failed launch too.
// launch(tp) enqueues the work; `what` names it in the message.
template <class Launch>
static int trace_set_launch(vrt_scene *s, float min_voxel, size_t rec_skip, size_t nslots, const char *what,
                            hipStream_t st, Launch launch)
{
        const int set = s->lm_cur;
        TraceParams tp0, tp;
        std::memset(&tp0, 0, sizeof tp0);
        tp0.r.sc = s->dev;
        tp0.r.test_flags = g_test_flags.load();
        fill_trace_light(s, set, min_voxel, &tp0);
        if (int rc = trace_scratch_n(s, set, tp0, rec_skip + nslots, &tp))
                return rc;
        tp.rec += 4 * rec_skip;
        if (int rc = ts_acquire(s, set, st))
                return rc;
        (void)hipGetLastError();  // a leftover error of an earlier call is not this launch's
        const hipError_t e = launch(tp);
        if (e != hipSuccess) {
                (void)ts_release(s, set, st);
                return fail(VRT_E_DEVICE, "%s launch failed: %s", what, hipGetErrorString(e));
        }
        if (tp.build_steps) {  // k_cone_steps is enqueued (steps_commit)
                s->ts[set].steps_key[0] = tp.mindist;
                s->ts[set].steps_key[1] = tp.maxdist;
        }
        return ts_release(s, set, st);
}

// Host arrays chunk by chunk through the staging s->tb (caller holds s->mu):
// m = min(n, chunk) elements of `in` (in_sz bytes each) at its front, behind
// them the output arrays that are laid out (m elements each, never more than
// one chunk).  Per chunk of c elements: stage in, enqueue(d_in, d_out, c) on
// the scene's stream, the outputs back, one host sync, host_step(h_out, c),
// and the caller's arrays are filled.  d_out[k] / h_out[k]: output k on the
// device / in the pinned copy, null when it is not laid out.
struct ChunkOut {
        void *host;   // the caller's array, or null
        size_t sz;    // bytes per element
        bool staged;  // laid out: the caller wants it, or the host step reads it
};
constexpr int kChunkOuts = 5;
template <class Enqueue, class HostStep>
static int chunked_host(vrt_scene *s, const void *in, size_t in_sz, int64_t n, int64_t chunk, const ChunkOut *out,
                        int nout, Enqueue enqueue, HostStep host_step)
{
        const int64_t m = std::min(n, chunk);
        const size_t in_bytes = (size_t)m * in_sz;
        size_t off[kChunkOuts], end = in_bytes;
        for (int k = 0; k < nout; ++k) {
                off[k] = end;
                end += out[k].staged ? (size_t)m * out[k].sz : 0;
        }
        HIPCHK(s->tb.grow(end, s->stream));
        char *d = s->tb.d.as<char>(), *h = s->tb.h.as<char>();
        char *d_out[kChunkOuts], *h_out[kChunkOuts];
        for (int k = 0; k < nout; ++k) {
                d_out[k] = out[k].staged ? d + off[k] : nullptr;
                h_out[k] = out[k].staged ? h + off[k] : nullptr;
        }
        for (int64_t b = 0; b < n; b += m) {
                const int64_t c = std::min(m, n - b);
                par_memcpy(h, static_cast<const char *>(in) + (size_t)b * in_sz, (size_t)c * in_sz);
                HIPCHK(hipMemcpyAsync(d, h, (size_t)c * in_sz, hipMemcpyHostToDevice, s->stream));
                if (int rc = enqueue(d, d_out, c))
                        return rc;
                HIPCHK(hipMemcpyAsync(h + in_bytes, d + in_bytes, end - in_bytes, hipMemcpyDeviceToHost, s->stream));
                HIPCHK(hipStreamSynchronize(s->stream));
                if (int rc = host_step(h_out, c))
                        return rc;
                for (int k = 0; k < nout; ++k)
                        if (out[k].host)
                                par_memcpy(static_cast<char *>(out[k].host) + (size_t)b * out[k].sz, h_out[k],
                                           (size_t)c * out[k].sz);
        }
        return VRT_OK;
}

// One batched trace() (io.rays set) or cone_trace (io.isects set) over device
// arrays on stream st.  trace() marches with even_invisible = true: the mixed
// march on a probe scene.
static int batch_enqueue(vrt_scene *s, const BatchIO &io, float min_voxel, hipStream_t st)
{
        const int64_t chunk = batch_chunk();
        const ProbeDev *pd = s->probes.empty() ? nullptr : &s->pdev;
        return trace_set_launch(s, min_voxel, 0, io.rays ? (size_t)std::min(io.n, chunk) : 0, "batched trace", st,
                                [&](const TraceParams &tp) {
                                        return io.rays ? launch_trace_batch(tp, io, chunk, st, pd)
                                                       : launch_cones_batch(tp, io, st);
                                });
}

extern "C" int vrt_trace_batch_device(vrt_scene *s, const vrt_ray *d_rays, int64_t n, float min_voxel,
                                      float *d_rgb, const vrt_trace_parts *d_parts, void *stream)
{
        std::unique_lock<std::mutex> lk;
        bool empty;
        if (int rc = batch_begin(s, n, d_rays && d_rgb, nullptr, 0, min_voxel, &lk, &empty); rc || empty)
                return rc;
        BatchIO io{};
        io.rays = reinterpret_cast<const float *>(d_rays);
        io.n = n;
        io.rgb = d_rgb;
        if (d_parts) {
                io.hits = reinterpret_cast<uint32_t *>(d_parts->hits);
                io.indirect = d_parts->indirect;
                io.direct = d_parts->direct;
                io.albedo = d_parts->albedo;
        }
        return batch_enqueue(s, io, min_voxel, static_cast<hipStream_t>(stream));
}

extern "C" int vrt_cone_trace_batch_device(vrt_scene *s, const vrt_isect *d_isects, int64_t n, float min_voxel,
                                           float *d_rgb, void *stream)
{
        std::unique_lock<std::mutex> lk;
        bool empty;
        if (int rc = batch_begin(s, n, d_isects && d_rgb, nullptr, 0, min_voxel, &lk, &empty); rc || empty)
                return rc;
        BatchIO io{};
        io.isects = reinterpret_cast<const float *>(d_isects);
        io.n = n;
        io.rgb = d_rgb;
        return batch_enqueue(s, io, min_voxel, static_cast<hipStream_t>(stream));
}

static void probe_shade(const vrt_scene *s, const vrt_hit *hits, int64_t n, float *rgb, float *albedo);
static int fetch_probe_sgs(vrt_scene *s);

// trace() (rays) or cone_trace over host arrays; out: rgb, hits, indirect,
// direct, albedo (caller holds s->mu)
static int batch_host(vrt_scene *s, const void *in, size_t in_sz, bool rays, int64_t n, float min_voxel,
                      void *const out[5])
{
        // trace() on a probe scene: the chunk's hit records come back
        // whether or not the caller asked for them, and the rays that ended
        // on a probe get their colour here (LightProbe::eval, the C
        // library's expf) before the chunk is handed out
        const bool shade = rays && !s->probes.empty();
        const ChunkOut co[5] = { { out[0], 12, true },
                                 { out[1], sizeof(vrt_hit), out[1] || shade },
                                 { out[2], 12, out[2] != nullptr },
                                 { out[3], 12, out[3] != nullptr },
                                 { out[4], 12, out[4] != nullptr } };
        return chunked_host(
                s, in, in_sz, n, batch_chunk(), co, 5,
                [&](char *d_in, char *const *d, int64_t c) {
                        BatchIO io{};
                        (rays ? io.rays : io.isects) = reinterpret_cast<const float *>(d_in);
                        io.n = c;
                        io.rgb = reinterpret_cast<float *>(d[0]);
                        io.hits = reinterpret_cast<uint32_t *>(d[1]);
                        io.indirect = reinterpret_cast<float *>(d[2]);
                        io.direct = reinterpret_cast<float *>(d[3]);
                        io.albedo = reinterpret_cast<float *>(d[4]);
                        return batch_enqueue(s, io, min_voxel, s->stream);
                },
                [&](char *const *h, int64_t c) {
                        if (!shade)
                                return (int)VRT_OK;
                        if (int rc = fetch_probe_sgs(s))  // a device gather may hold the latest SGs
                                return rc;
                        probe_shade(s, reinterpret_cast<const vrt_hit *>(h[1]), c, reinterpret_cast<float *>(h[0]),
                                    reinterpret_cast<float *>(h[4]));
                        return (int)VRT_OK;
                });
}

extern "C" int vrt_trace_batch(vrt_scene *s, const vrt_ray *rays, int64_t n, float min_voxel, float *rgb,
                               const vrt_trace_parts *parts)
{
        static_assert(sizeof(vrt_isect) == 24, "vrt_isect layout");
        std::unique_lock<std::mutex> lk;
        bool empty;
        if (int rc = batch_begin(s, n, rays && rgb, nullptr, 0, min_voxel, &lk, &empty); rc || empty)
                return rc;
        void *const out[5] = { rgb, parts ? parts->hits : nullptr, parts ? parts->indirect : nullptr,
                               parts ? parts->direct : nullptr, parts ? parts->albedo : nullptr };
        return batch_host(s, rays, sizeof(vrt_ray), true, n, min_voxel, out);
}

extern "C" int vrt_cone_trace_batch(vrt_scene *s, const vrt_isect *isects, int64_t n, float min_voxel, float *rgb)
{
        std::unique_lock<std::mutex> lk;
        bool empty;
        if (int rc = batch_begin(s, n, isects && rgb, nullptr, 0, min_voxel, &lk, &empty); rc || empty)
                return rc;
        void *const out[5] = { rgb, nullptr, nullptr, nullptr, nullptr };
        return batch_host(s, isects, sizeof(vrt_isect), false, n, min_voxel, out);
}

// ---- light probes (gi::LightProbe, gi::SG; VRT/voxel_octree.cc:497-632) ----
// jql::PCG::operator() (VRT/graphics_math.h:839-853)
static uint32_t pcg_next_host(uint64_t &s)
{
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        const uint32_t xorshift = (uint32_t)((s ^ (s >> 18u)) >> 27u);
        const uint32_t shift = (uint32_t)(s >> 59u);
        return (xorshift >> shift) | (xorshift << ((0u - shift) & 31u));
}

// libstdc++'s uniform_real_distribution<float>{-1, 1} over a 32-bit
// generator: generate_canonical<float, 24> = float(g) / 2^32 (below 1), then
// u * (1 - -1) + -1 -- the mapping the config-5 kernels use
static float uniform_m11_host(uint64_t &s)
{
        float sum = 0.0f;
        sum += (float)pcg_next_host(s) * 1.0f;
        float ret = sum / 4294967296.0f;
        if (ret >= 1.0f)
                ret = 0.99999994f;  // nextafter(1.f, 0.f)
        return (ret * (1.0f - -1.0f)) + -1.0f;
}

// jql::random_point_in_unit_sphere (VRT/graphics_math.h:1208-1216): three
// draws in x, y, z order until length(r) < 1
static void probe_points_host(uint64_t seed, int n, float *pts)
{
        uint64_t st = seed;
        for (int i = 0; i < n; ++i)
                for (;;) {
                        const float x = uniform_m11_host(st);
                        const float y = uniform_m11_host(st);
                        const float z = uniform_m11_host(st);
                        if (length(mk3(x, y, z)) < 1.f) {
                                pts[3 * i + 0] = x;
                                pts[3 * i + 1] = y;
                                pts[3 * i + 2] = z;
                                break;
                        }
                }
}

extern "C" int vrt_probe_points(uint64_t seed, int n, float *pts)
{
        if (!pts || n < 1 || n > kProbeMaxPoints)
                return fail(VRT_E_INVALID, "bad argument: %d points (1..%d)", n, kProbeMaxPoints);
        probe_points_host(seed, n, pts);
        return VRT_OK;
}

// LightProbe::eval (VRT/voxel_octree.cc:626-632): the 14 lobes' SG::eval
// a * expf(s * (dot(dir, d) - 1)) (:503-508) added in order from zero
extern "C" int vrt_probe_eval(const vrt_sg *sgs, int64_t n, const float *dirs, int64_t m, float *rgb)
{
        static_assert(sizeof(vrt_sg) == 28, "vrt_sg layout");
        static_assert(sizeof(vrt_probe) == 16, "vrt_probe layout");
        static_assert(kProbeSGs == VRT_PROBE_SGS && kProbeMaxPoints == VRT_PROBE_MAX_POINTS, "vrt.h constants");
        if (n < 0 || m < 0)
                return fail(VRT_E_INVALID, "bad argument");
        if (n == 0 || m == 0)
                return VRT_OK;
        if (!sgs || !dirs || !rgb)
                return fail(VRT_E_INVALID, "null argument");
        for (int64_t pi = 0; pi < n; ++pi)
                for (int64_t k = 0; k < m; ++k) {
                        const f3 dir = mk3(dirs[3 * k], dirs[3 * k + 1], dirs[3 * k + 2]);
                        f3 lit = mk3(0.f, 0.f, 0.f);
                        for (int i = 0; i < VRT_PROBE_SGS; ++i) {
                                const vrt_sg &g = sgs[pi * VRT_PROBE_SGS + i];
                                const float tmp = dot(dir, mk3(g.d[0], g.d[1], g.d[2]));
                                const float e = expf(g.s * (tmp - 1));
                                lit = lit + mk3(g.a[0], g.a[1], g.a[2]) * e;
                        }
                        float *o = rgb + (pi * m + k) * 3;
                        o[0] = lit.x;
                        o[1] = lit.y;
                        o[2] = lit.z;
                }
        return VRT_OK;
}

// probes per chunk: 14 * npoints records each in the set's record block
static int64_t probe_chunk(int npoints)
{
        if (g_test_flags.load() & VRT_TEST_SMALL_PROBE_CHUNK)
                return 2;
        return std::max<int64_t>(1, kBatchChunk / ((int64_t)kProbeSGs * npoints));
}

// One gather on stream st over device arrays, as batch_enqueue.  rec_skip:
// records at the front of the set's block that belong to a frame in flight
// (vrt_trace_frame_probes_device: the view's primary records, which the cones
// + film pass reads after this gather); the gather's own follow them.
static int probe_enqueue(vrt_scene *s, const ProbeIO &io0, const float *host_points, float min_voxel,
                         hipStream_t st, size_t rec_skip = 0)
{
        ProbeIO io = io0;
        io.res = min_voxel;
        if (!(io.res > 0.f))
                vrt_scene_min_voxel(s, 0, &io.res);
        const int64_t chunk = probe_chunk(io.npoints);
        return trace_set_launch(s, min_voxel, rec_skip, (size_t)std::min(io.n, chunk) * kProbeSGs * io.npoints,
                                "probe gather", st, [&](const TraceParams &tp) {
                                        return launch_probe_gather(tp, io, host_points, chunk, st);
                                });
}

// the reference's own points (every LightProbe draws the same 100)
static const float *probe_default_points()
{
        static const std::vector<float> pts = [] {
                std::vector<float> v(300);
                probe_points_host(0xc01dbeefULL, 100, v.data());
                return v;
        }();
        return pts.data();
}

extern "C" int vrt_probe_gather_device(vrt_scene *s, const vrt_probe *d_probes, int64_t n, float min_voxel,
                                       const float light_color[3], const float *points, int npoints,
                                       vrt_sg *d_sgs, float *d_terms, void *stream)
{
        std::unique_lock<std::mutex> lk;
        bool empty;
        if (int rc = batch_begin(s, n, d_probes && light_color && d_sgs, points, npoints, min_voxel, &lk, &empty);
            rc || empty)
                return rc;
        ProbeIO io{};
        io.probes = reinterpret_cast<const float *>(d_probes);
        io.n = n;
        io.npoints = points ? npoints : 100;
        std::memcpy(io.light, light_color, sizeof io.light);
        io.sgs = reinterpret_cast<float *>(d_sgs);
        io.terms = d_terms;
        return probe_enqueue(s, io, points ? points : probe_default_points(), min_voxel,
                             static_cast<hipStream_t>(stream));
}

// Host arrays: chunk by chunk through the batched trace's staging (one
// chunk's probes, SGs and terms).
extern "C" int vrt_probe_gather(vrt_scene *s, const vrt_probe *probes, int64_t n, float min_voxel,
                                const float light_color[3], const float *points, int npoints, vrt_sg *sgs,
                                float *terms)
{
        std::unique_lock<std::mutex> lk;
        bool empty;
        if (int rc = batch_begin(s, n, probes && light_color && sgs, points, npoints, min_voxel, &lk, &empty);
            rc || empty)
                return rc;
        const int np = points ? npoints : 100;
        const float *pts = points ? points : probe_default_points();
        const ChunkOut co[2] = { { sgs, (size_t)kProbeSGs * sizeof(vrt_sg), true },
                                 { terms, (size_t)kProbeSGs * np * 12, terms != nullptr } };
        return chunked_host(
                s, probes, sizeof(vrt_probe), n, probe_chunk(np), co, 2,
                [&](char *d_in, char *const *d, int64_t c) {
                        ProbeIO io{};
                        io.probes = reinterpret_cast<const float *>(d_in);
                        io.n = c;
                        io.npoints = np;
                        std::memcpy(io.light, light_color, sizeof io.light);
                        io.sgs = reinterpret_cast<float *>(d[0]);
                        io.terms = reinterpret_cast<float *>(d[1]);
                        return probe_enqueue(s, io, pts, min_voxel, s->stream);
                },
                [](char *const *, int64_t) { return (int)VRT_OK; });
}

// ---- light probes as scene voxels (vrt_scene_create_probes) ----------------
extern "C" int vrt_probe_overlap(const vrt_probe *p, const float box[6])
{
        if (!p || !box)
                return fail(VRT_E_INVALID, "null argument");
        return probe_overlap(mk3(p->o[0], p->o[1], p->o[2]), p->r, box, box + 3) ? 1 : 0;
}

extern "C" int vrt_probe_isect(const vrt_probe *p, const vrt_ray *ray, const float prev_hit[3], float *t,
                               float hit_p[3], float normal[3])
{
        if (!p || !ray || !prev_hit || !t || !hit_p || !normal)
                return fail(VRT_E_INVALID, "null argument");
        float tt;
        f3 hp, nrm;
        if (!probe_isect(mk3(p->o[0], p->o[1], p->o[2]), p->r, mk3(ray->o[0], ray->o[1], ray->o[2]),
                         mk3(ray->d[0], ray->d[1], ray->d[2]), mk3(prev_hit[0], prev_hit[1], prev_hit[2]), &tt, &hp,
                         &nrm))
                return 0;
        *t = tt;
        hit_p[0] = hp.x, hit_p[1] = hp.y, hit_p[2] = hp.z;
        normal[0] = nrm.x, normal[1] = nrm.y, normal[2] = nrm.z;
        return 1;
}

extern "C" int vrt_scene_probe_info(const vrt_scene *s, int32_t *nprobe, int64_t *probe_leaves, int64_t *probe_refs)
{
        if (!s)
                return fail(VRT_E_INVALID, "null argument");
        if (nprobe)
                *nprobe = (int32_t)s->probes.size();
        if (probe_leaves)
                *probe_leaves = s->probe_leaves;
        if (probe_refs)
                *probe_refs = (int64_t)s->pref.size();
        return VRT_OK;
}

extern "C" int vrt_scene_probe_leaves(const vrt_scene *s, uint32_t *voxel, uint32_t *count, int32_t *probes)
{
        if (!s || !voxel || !count || !probes)
                return fail(VRT_E_INVALID, "null argument");
        std::vector<std::pair<uint32_t, size_t>> lv;
        for (size_t i = 0; i < s->pnode.size(); ++i)
                if ((s->nodes[i].a & kLeafBit) && s->pnode[i].y)
                        lv.emplace_back(s->node_vox[i], i);
        std::sort(lv.begin(), lv.end());
        size_t o = 0;
        for (size_t j = 0; j < lv.size(); ++j) {
                const uint2 pn = s->pnode[lv[j].second];
                voxel[j] = lv[j].first;
                count[j] = pn.y;
                for (uint32_t k = 0; k < pn.y; ++k)
                        probes[o++] = (int32_t)s->pref[pn.x + k];
        }
        return VRT_OK;
}

// The stored SGs live twice: probe_sgs on the host (vrt_probe_shade_hits,
// the host-array trace batch) and d_sgs on the device (the kernels that shade
// a probe hit).  Whoever changes one copy brings the other up to date before
// its next reader; both helpers first wait for the scene's work in flight --
// the scene stream and each trace set's last user, through which every reader
// and writer of d_sgs is ordered.  Caller holds s->mu.
static int probe_sgs_quiesce(vrt_scene *s)
{
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(hipStreamSynchronize(s->stream));
        for (TraceSet &t : s->ts)
                HIPCHK(t.use.sync());
        return VRT_OK;
}

// the host copy changed (vrt_scene_set_probe_sgs, vrt_scene_probes_gather)
static int upload_probe_sgs(vrt_scene *s)
{
        s->sgs_stale = false;
        if (!s->d_sgs)
                return VRT_OK;
        if (int rc = probe_sgs_quiesce(s))
                return rc;
        HIPCHK(hipMemcpy(s->d_sgs, s->probe_sgs.data(), s->probe_sgs.size() * sizeof(vrt_sg), hipMemcpyHostToDevice));
        return VRT_OK;
}

// a device gather wrote d_sgs last (sgs_stale): fetch before a host reader
static int fetch_probe_sgs(vrt_scene *s)
{
        if (!s->sgs_stale || !s->d_sgs)
                return VRT_OK;
        if (int rc = probe_sgs_quiesce(s))
                return rc;
        HIPCHK(hipMemcpy(s->probe_sgs.data(), s->d_sgs, s->probe_sgs.size() * sizeof(vrt_sg), hipMemcpyDeviceToHost));
        s->sgs_stale = false;
        return VRT_OK;
}

extern "C" int vrt_scene_set_probe_sgs(vrt_scene *s, const vrt_sg *sgs)
{
        if (!s || !sgs)
                return fail(VRT_E_INVALID, "null argument");
        if (s->probes.empty())
                return fail(VRT_E_INVALID, "the scene has no probes (vrt_scene_create_probes)");
        std::lock_guard<std::mutex> lk(s->mu);
        std::copy(sgs, sgs + s->probe_sgs.size(), s->probe_sgs.begin());
        return upload_probe_sgs(s);
}

extern "C" int vrt_scene_probe_sgs(const vrt_scene *s, vrt_sg *sgs)
{
        if (!s || !sgs)
                return fail(VRT_E_INVALID, "null argument");
        if (s->probes.empty())
                return fail(VRT_E_INVALID, "the scene has no probes (vrt_scene_create_probes)");
        vrt_scene *ms = const_cast<vrt_scene *>(s);
        std::lock_guard<std::mutex> lk(ms->mu);
        if (int rc = fetch_probe_sgs(ms))  // a device gather may hold the latest
                return rc;
        std::copy(s->probe_sgs.begin(), s->probe_sgs.end(), sgs);
        return VRT_OK;
}

extern "C" int vrt_scene_probes_gather(vrt_scene *s, float min_voxel, const float light_color[3])
{
        if (!s || !light_color)
                return fail(VRT_E_INVALID, "null argument");
        if (s->probes.empty())
                return fail(VRT_E_INVALID, "the scene has no probes (vrt_scene_create_probes)");
        // VRT/main.cc:104-105: every probe's gather_light with its own 100 points
        std::vector<vrt_sg> sgs(s->probe_sgs.size());
        if (int rc = vrt_probe_gather(s, s->probes.data(), (int64_t)s->probes.size(), min_voxel, light_color, nullptr,
                                      100, sgs.data(), nullptr))
                return rc;
        std::lock_guard<std::mutex> lk(s->mu);
        s->probe_sgs.swap(sgs);
        return upload_probe_sgs(s);
}

// LightProbe::get_albedo (VRT/voxel_octree.cc:562-566) for the elements of a
// batch that ended on a probe: eval(normalize(hit - o_)) over the stored SGs,
// vrt_probe_eval's code; albedo = rgb (trace() returns get_albedo itself)
static void probe_shade(const vrt_scene *s, const vrt_hit *hits, int64_t n, float *rgb, float *albedo)
{
        const int64_t np = (int64_t)s->probes.size();
        for (int64_t i = 0; i < n; ++i) {
                const vrt_hit &h = hits[i];
                const int64_t k = (int64_t)h.tri - s->ntri;
                if (h.hit != 1 || k < 0 || k >= np)
                        continue;
                const vrt_probe &pb = s->probes[(size_t)k];
                const f3 dir = normalize(mk3(h.hit_p[0], h.hit_p[1], h.hit_p[2]) - mk3(pb.o[0], pb.o[1], pb.o[2]));
                const float dv[3] = { dir.x, dir.y, dir.z };
                float c[3];
                vrt_probe_eval(&s->probe_sgs[(size_t)k * kProbeSGs], 1, dv, 1, c);
                for (int q = 0; q < 3; ++q) {
                        if (rgb)
                                rgb[3 * i + q] = c[q];
                        if (albedo)
                                albedo[3 * i + q] = c[q];
                }
        }
}

extern "C" int vrt_probe_shade_hits(vrt_scene *s, const vrt_hit *hits, int64_t n, float *rgb, float *albedo)
{
        if (!s || n < 0 || (n > 0 && !hits))
                return fail(VRT_E_INVALID, "bad argument");
        std::lock_guard<std::mutex> lk(s->mu);
        if (int rc = fetch_probe_sgs(s))
                return rc;
        probe_shade(s, hits, n, rgb, albedo);
        return VRT_OK;
}

// ---- probe hits shaded on the device ---------------------------------------
// The C library's expf through a volatile argument: the compiler can neither
// fold the call nor replace it.
static float libm_expf(float x)
{
        volatile float xv = x;
        return expf(xv);
}

static float bits_f32(uint32_t u)
{
        float f;
        std::memcpy(&f, &u, 4);
        return f;
}

// host threads of the expf sweeps: never more than 16, whatever the machine has
static int expf_pool()
{
        const unsigned h = std::thread::hardware_concurrency();
        return (int)std::min(16u, std::max(1u, h));
}

// f(begin, end) over [0, n) split evenly over the pool
static void expf_parallel(uint64_t n, const std::function<void(int, uint64_t, uint64_t)> &f)
{
        const int nt = (int)std::min<uint64_t>((uint64_t)expf_pool(), std::max<uint64_t>(1, n >> 16));
        if (nt <= 1) {
                f(0, 0, n);
                return;
        }
        std::vector<std::thread> th;
        for (int t = 0; t < nt; ++t)
                th.emplace_back(f, t, n * (uint64_t)t / nt, n * (uint64_t)(t + 1) / nt);
        for (auto &x : th)
                x.join();
}

// The inputs that tell the flavours apart and an unknown libm from both: the
// two floats at which the flavours differ, the special-case boundaries, and
// 960 mantissas in every binade of [2^-27, 128) for both signs (65,280).
static std::vector<float> expf_probe_inputs()
{
        std::vector<float> v = { 0x1.04845ep+5f, -0x1.f8cbb2p+5f, 0.f, -0.f, 88.0f, -88.0f,
                                 0x1.62e42ep6f, 0x1.62e43p6f, 0x1.62e42cp6f,
                                 -0x1.9fe368p6f, -0x1.9fe36ap6f, -0x1.9fe366p6f, -0x1.9d1d9ep6f,
                                 std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(),
                                 std::numeric_limits<float>::denorm_min(), -std::numeric_limits<float>::denorm_min() };
        for (uint32_t e = 127 - 27; e < 127 + 7; ++e)
                for (uint32_t j = 0; j < 960; ++j) {
                        const uint32_t m = j * 8738u + ((j * 37u) & 0xFFu);
                        v.push_back(bits_f32((e << 23) | m));
                        v.push_back(bits_f32(0x80000000u | (e << 23) | m));
                }
        return v;
}

static int expf_flavour_cached()
{
        static std::mutex mu;
        static int flavour = -2;
        std::lock_guard<std::mutex> lk(mu);
        if (flavour == -2) {
                bool is[2] = { true, true };
                for (float x : expf_probe_inputs()) {
                        const uint32_t ref = f32_bits(libm_expf(x));
                        is[0] = is[0] && ref == f32_bits(expf_model(x, false));
                        is[1] = is[1] && ref == f32_bits(expf_model(x, true));
                }
                flavour = is[1] ? 1 : is[0] ? 0 : -1;
        }
        return flavour;
}

extern "C" int vrt_expf_flavour(int *flavour)
{
        if (!flavour)
                return fail(VRT_E_INVALID, "null argument");
        *flavour = expf_flavour_cached();
        return VRT_OK;
}

extern "C" int vrt_expf_model(const float *x, int64_t n, int flavour, float *y)
{
        if (n < 0 || (n > 0 && (!x || !y)) || (flavour != 0 && flavour != 1))
                return fail(VRT_E_INVALID, "bad argument");
        for (int64_t i = 0; i < n; ++i)
                y[i] = expf_model(x[i], flavour == 1);
        return VRT_OK;
}

// the kernels' model on host arrays (either flavour, whatever libm is)
extern "C" int vrt_expf_model_device(int device, const float *x, int64_t n, int flavour, float *y)
{
        if (n < 0 || (n > 0 && (!x || !y)) || (flavour != 0 && flavour != 1))
                return fail(VRT_E_INVALID, "bad argument");
        if (int rc = check_device(device))
                return rc;
        if (n == 0)
                return VRT_OK;
        HIPCHK(hipSetDevice(device));
        DevMem dx, dy;
        HIPCHK(dx.alloc((size_t)n * 4));
        HIPCHK(dy.alloc((size_t)n * 4));
        HIPCHK(hipMemcpy(dx, x, (size_t)n * 4, hipMemcpyHostToDevice));
        HIPCHK(launch_expf_model(dx.as<float>(), n, flavour, dy.as<float>(), nullptr));
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(y, dy, (size_t)n * 4, hipMemcpyDeviceToHost));
        return VRT_OK;
}

// patterns k0 .. k0 + cnt of the sweep against libm: dev = the kernel's
// results for them (nullptr: the host model); adds to *bad, lowers *first_k
static void expf_compare(uint32_t first, uint32_t stride, uint64_t k0, uint64_t cnt, int flavour, const float *dev,
                         uint64_t *bad, uint64_t *first_k)
{
        std::mutex mu;
        expf_parallel(cnt, [&](int, uint64_t b, uint64_t e) {
                uint64_t nb = 0, fk = UINT64_MAX;
                for (uint64_t j = b; j < e; ++j) {
                        const uint32_t u = first + (uint32_t)(k0 + j) * stride;
                        const float x = bits_f32(u);
                        if (x != x)
                                continue;
                        const float got = dev ? dev[j] : expf_model(x, flavour == 1);
                        if (f32_bits(got) != f32_bits(libm_expf(x))) {
                                if (!nb)
                                        fk = k0 + j;
                                ++nb;
                        }
                }
                std::lock_guard<std::mutex> lk(mu);
                *bad += nb;
                *first_k = std::min(*first_k, fk);
        });
}

extern "C" int vrt_expf_selftest(int device, uint32_t first_bits, uint64_t count, uint32_t stride, int flavour,
                                 uint64_t *mismatches, uint32_t *first_bad)
{
        if (!mismatches || (flavour != 0 && flavour != 1))
                return fail(VRT_E_INVALID, "bad argument");
        uint64_t bad = 0, first_k = UINT64_MAX;
        if (device < 0) {
                expf_compare(first_bits, stride, 0, count, flavour, nullptr, &bad, &first_k);
        } else {
                if (int rc = check_device(device))
                        return rc;
                HIPCHK(hipSetDevice(device));
                // two chunks in flight: the kernel and the copy of chunk c run
                // while the host compares chunk c - 1
                constexpr uint64_t kChunk = (uint64_t)1 << 24;
                const uint64_t m = std::min(count, kChunk);
                struct {
                        DevMem d[2];
                        PinnedMem h[2];
                        Stream st;
                } bf;
                if (count > 0) {
                        HIPCHK(bf.st.create());
                        for (int k = 0; k < (count > kChunk ? 2 : 1); ++k) {
                                HIPCHK(bf.d[k].alloc(m * 4));
                                HIPCHK(bf.h[k].alloc(m * 4));
                        }
                }
                auto enqueue = [&](uint64_t k0) -> int {
                        const int b = (int)((k0 / kChunk) & 1);
                        const uint64_t c = std::min(kChunk, count - k0);
                        HIPCHK(launch_selftest_expf(first_bits + (uint32_t)k0 * stride, stride, (int64_t)c, flavour,
                                                    bf.d[b].as<float>(), bf.st));
                        HIPCHK(hipMemcpyAsync(bf.h[b], bf.d[b], c * 4, hipMemcpyDeviceToHost, bf.st));
                        return VRT_OK;
                };
                if (count > 0)
                        if (int rc = enqueue(0))
                                return rc;
                for (uint64_t k0 = 0; k0 < count; k0 += kChunk) {
                        // chunk k0 is the only work on the stream here
                        HIPCHK(hipStreamSynchronize(bf.st));
                        if (k0 + kChunk < count)
                                if (int rc = enqueue(k0 + kChunk))
                                        return rc;
                        expf_compare(first_bits, stride, k0, std::min(kChunk, count - k0), flavour,
                                     bf.h[(k0 / kChunk) & 1].as<float>(), &bad, &first_k);
                }
        }
        *mismatches = bad;
        if (bad && first_bad)
                *first_bad = first_bits + (uint32_t)first_k * stride;
        return VRT_OK;
}

// the detected flavour for a device-shading call, or VRT_E_INVALID
static int device_expf(const char *what, int *fused)
{
        const int f = expf_flavour_cached();
        if (f < 0)
                return fail(VRT_E_INVALID,
                            "%s: this C library's expf is neither flavour of the device model; shade probe hits on "
                            "the host with vrt_probe_shade_hits",
                            what);
        *fused = f;
        return VRT_OK;
}

extern "C" int vrt_probe_eval_device(int device, const vrt_sg *d_sgs, int64_t n, const float *d_dirs, int64_t m,
                                     float *d_rgb, void *stream)
{
        if (n < 0 || m < 0 || (n > 0 && m > 0 && n > INT64_MAX / 3 / m))
                return fail(VRT_E_INVALID, "bad argument");
        if (n == 0 || m == 0)
                return VRT_OK;
        if (!d_sgs || !d_dirs || !d_rgb)
                return fail(VRT_E_INVALID, "null argument");
        int fused;
        if (int rc = device_expf("vrt_probe_eval_device", &fused))
                return rc;
        if (int rc = check_device(device))
                return rc;
        HIPCHK(hipSetDevice(device));
        HIPCHK(launch_probe_eval(reinterpret_cast<const float *>(d_sgs), n, d_dirs, m, fused, d_rgb,
                                 static_cast<hipStream_t>(stream)));
        return VRT_OK;
}

extern "C" int vrt_probe_shade_hits_device(vrt_scene *s, const vrt_hit *d_hits, int64_t n, float *d_rgb,
                                           float *d_albedo, void *stream)
{
        if (!s || n < 0 || (n > 0 && !d_hits))
                return fail(VRT_E_INVALID, "bad argument");
        if (n == 0 || s->probes.empty() || (!d_rgb && !d_albedo))
                return VRT_OK;
        if (need_device(s))
                return VRT_E_NODEVICE;
        int fused;
        if (int rc = device_expf("vrt_probe_shade_hits_device", &fused))
                return rc;
        std::lock_guard<std::mutex> lk(s->mu);
        HIPCHK(hipSetDevice(s->device));
        hipStream_t st = static_cast<hipStream_t>(stream);
        // behind the batch that wrote the hits, and a reader of the device SGs:
        // through the trace sets' events, as vrt_trace_batch_device is
        const int set = s->lm_cur >= 0 ? s->lm_cur : 0;
        for (int k = 0; k < 2; ++k)
                if (int rc = ts_acquire(s, k, st))
                        return rc;
        (void)hipGetLastError();
        const hipError_t e = launch_probe_shade_hits(d_hits, n, s->pdev, (int32_t)s->probes.size(), s->d_sgs, fused,
                                                     d_rgb, d_albedo, st);
        if (e != hipSuccess)
                return fail(VRT_E_DEVICE, "probe shading launch failed: %s", hipGetErrorString(e));
        return ts_release(s, set, st);
}

// ---- the SG algebra and the probes' irradiance (vrt_sg.h) -------------------
// the host calls' expf: the C library's
struct LibmExp {
        float operator()(float x) const { return expf(x); }
};

// n and the arrays of a batched SG call: VRT_OK with *empty set for n == 0
static int sg_args(int64_t n, bool arrays, bool *empty)
{
        static_assert(sizeof(vrt_sg) == 28 && sizeof(vrt_isect) == 24, "vrt_sg / vrt_isect layout");
        *empty = n == 0;
        if (n < 0)
                return fail(VRT_E_INVALID, "bad argument: n = %lld", (long long)n);
        if (n > 0 && !arrays)
                return fail(VRT_E_INVALID, "null argument");
        return VRT_OK;
}

static const float *sg_f(const vrt_sg *p) { return reinterpret_cast<const float *>(p); }
static float *sg_f(vrt_sg *p) { return reinterpret_cast<float *>(p); }

extern "C" int vrt_sg_make(const float *a, const float *d, const float *s, int64_t n, vrt_sg *out)
{
        bool empty;
        if (int rc = sg_args(n, a && d && s && out, &empty); rc || empty)
                return rc;
        for (int64_t i = 0; i < n; ++i)
                sg_store(sg_f(out) + 7 * i, sg_make(mk3(a[3 * i], a[3 * i + 1], a[3 * i + 2]),
                                                    mk3(d[3 * i], d[3 * i + 1], d[3 * i + 2]), s[i]));
        return VRT_OK;
}

extern "C" int vrt_sg_integral(const vrt_sg *sgs, int64_t n, float *rgb)
{
        bool empty;
        if (int rc = sg_args(n, sgs && rgb, &empty); rc || empty)
                return rc;
        for (int64_t i = 0; i < n; ++i)
                f3_store(rgb + 3 * i, sg_integral(sg_load(sg_f(sgs) + 7 * i), LibmExp{}));
        return VRT_OK;
}

extern "C" int vrt_sg_prod(const vrt_sg *lhs, const vrt_sg *rhs, int64_t n, vrt_sg *out)
{
        bool empty;
        if (int rc = sg_args(n, lhs && rhs && out, &empty); rc || empty)
                return rc;
        for (int64_t i = 0; i < n; ++i)
                sg_store(sg_f(out) + 7 * i,
                         sg_prod(sg_load(sg_f(lhs) + 7 * i), sg_load(sg_f(rhs) + 7 * i), LibmExp{}));
        return VRT_OK;
}

extern "C" int vrt_sg_inner_prod(const vrt_sg *lhs, const vrt_sg *rhs, int64_t n, float *rgb)
{
        bool empty;
        if (int rc = sg_args(n, lhs && rhs && rgb, &empty); rc || empty)
                return rc;
        for (int64_t i = 0; i < n; ++i)
                f3_store(rgb + 3 * i,
                         sg_inner_prod(sg_load(sg_f(lhs) + 7 * i), sg_load(sg_f(rhs) + 7 * i), LibmExp{}));
        return VRT_OK;
}

// what the three device calls share: arguments, the expf flavour, the device
static int sg_device_begin(const char *what, int device, int64_t n, bool arrays, int *fused, bool *empty)
{
        if (int rc = sg_args(n, arrays, empty); rc || *empty)
                return rc;
        if (int rc = device_expf(what, fused))
                return rc;
        if (int rc = check_device(device))
                return rc;
        HIPCHK(hipSetDevice(device));
        return VRT_OK;
}

extern "C" int vrt_sg_integral_device(int device, const vrt_sg *d_sgs, int64_t n, float *d_rgb, void *stream)
{
        int fused;
        bool empty;
        if (int rc = sg_device_begin("vrt_sg_integral_device", device, n, d_sgs && d_rgb, &fused, &empty); rc || empty)
                return rc;
        HIPCHK(launch_sg_integral(sg_f(d_sgs), n, fused, d_rgb, static_cast<hipStream_t>(stream)));
        return VRT_OK;
}

extern "C" int vrt_sg_prod_device(int device, const vrt_sg *d_lhs, const vrt_sg *d_rhs, int64_t n, vrt_sg *d_out,
                                  void *stream)
{
        int fused;
        bool empty;
        if (int rc = sg_device_begin("vrt_sg_prod_device", device, n, d_lhs && d_rhs && d_out, &fused, &empty);
            rc || empty)
                return rc;
        HIPCHK(launch_sg_prod(sg_f(d_lhs), sg_f(d_rhs), n, fused, sg_f(d_out), static_cast<hipStream_t>(stream)));
        return VRT_OK;
}

extern "C" int vrt_sg_inner_prod_device(int device, const vrt_sg *d_lhs, const vrt_sg *d_rhs, int64_t n,
                                        float *d_rgb, void *stream)
{
        int fused;
        bool empty;
        if (int rc = sg_device_begin("vrt_sg_inner_prod_device", device, n, d_lhs && d_rhs && d_rgb, &fused, &empty);
            rc || empty)
                return rc;
        HIPCHK(launch_sg_inner_prod(sg_f(d_lhs), sg_f(d_rhs), n, fused, d_rgb, static_cast<hipStream_t>(stream)));
        return VRT_OK;
}

// the arguments of both irradiance calls
static int irradiance_args(const vrt_scene *s, const vrt_isect *isects, int64_t n, const float *lobe_a,
                           const float *rgb, bool *empty)
{
        if (!s)
                return fail(VRT_E_INVALID, "null argument");
        if (s->probes.empty())
                return fail(VRT_E_INVALID, "the scene has no probes (vrt_scene_create_probes)");
        return sg_args(n, isects && lobe_a && rgb, empty);
}

// On the host from the scene's host arrays, whatever the scene's device is.
extern "C" int vrt_probe_irradiance(vrt_scene *s, const vrt_isect *isects, int64_t n, const float lobe_a[3],
                                    float lobe_s, float *rgb, int32_t *count)
{
        bool empty;
        if (int rc = irradiance_args(s, isects, n, lobe_a, rgb, &empty); rc || empty)
                return rc;
        std::lock_guard<std::mutex> lk(s->mu);
        if (int rc = fetch_probe_sgs(s))  // a device gather may hold the latest
                return rc;
        const f3 la = mk3(lobe_a[0], lobe_a[1], lobe_a[2]);
        const float *sgs = sg_f(s->probe_sgs.data());
        const float *isf = reinterpret_cast<const float *>(isects);
        const unsigned h = std::thread::hardware_concurrency();
        const int nt = (int)std::min<int64_t>(std::min(16u, std::max(1u, h)), std::max<int64_t>(1, n >> 12));
        auto work = [&](int64_t b, int64_t e) {
                for (int64_t i = b; i < e; ++i) {
                        f3 c;
                        const int32_t k = probe_irradiance_one(s->nodes.data(), s->pnode.data(), s->pref.data(), sgs,
                                                               isf + 6 * i, la, lobe_s, LibmExp{}, &c);
                        f3_store(rgb + 3 * i, c);
                        if (count)
                                count[i] = k;
                }
        };
        if (nt <= 1) {
                work(0, n);
                return VRT_OK;
        }
        std::vector<std::thread> th;
        for (int t = 0; t < nt; ++t)
                th.emplace_back(work, n * t / nt, n * (t + 1) / nt);
        for (auto &x : th)
                x.join();
        return VRT_OK;
}

extern "C" int vrt_probe_irradiance_device(vrt_scene *s, const vrt_isect *d_isects, int64_t n, const float lobe_a[3],
                                           float lobe_s, float *d_rgb, int32_t *d_count, void *stream)
{
        bool empty;
        if (int rc = irradiance_args(s, d_isects, n, lobe_a, d_rgb, &empty); rc || empty)
                return rc;
        if (need_device(s))
                return VRT_E_NODEVICE;
        int fused;
        if (int rc = device_expf("vrt_probe_irradiance_device", &fused))
                return rc;
        std::lock_guard<std::mutex> lk(s->mu);
        HIPCHK(hipSetDevice(s->device));
        hipStream_t st = static_cast<hipStream_t>(stream);
        // a reader of the device SGs: behind their writers (a frame's gather)
        // through the trace sets' events, as vrt_probe_shade_hits_device is
        const int set = s->lm_cur >= 0 ? s->lm_cur : 0;
        for (int k = 0; k < 2; ++k)
                if (int rc = ts_acquire(s, k, st))
                        return rc;
        (void)hipGetLastError();
        const hipError_t e = launch_probe_irradiance(s->dev.nodes, s->pdev, s->d_sgs,
                                                     reinterpret_cast<const float *>(d_isects), n, lobe_a, lobe_s,
                                                     fused, d_rgb, d_count, st);
        if (e != hipSuccess)
                return fail(VRT_E_DEVICE, "probe irradiance launch failed: %s", hipGetErrorString(e));
        return ts_release(s, set, st);
}

// ---- the trace() frames ----------------------------------------------------
// vrt_render_trace[_device] and vrt_trace_frame_device and, beside each, the
// _probes name that also serves a scene with light probes: one implementation
// per pair.  FramePath: what the call is (`what`, for its messages), whether
// it may take the probe path (a _probes name) and, from frame_args_ok,
// whether it does (a probe scene: the mixed primary march, probe hits shaded
// over the device SGs with the detected expf flavour `fused`).  On a triangle
// scene a _probes name is the old one.
struct FramePath {
        const char *what;
        bool may_probe;
        bool probe = false;
        int fused = 0;
};

// The frame calls' arguments, in one order for all six.  ptrs: the call's
// pointer arguments are all set; light_film: the frame calls' (has_light).
static int frame_args_ok(vrt_scene *s, FramePath *fp, bool ptrs, bool has_light, const vrt_film *light_film,
                         const vrt_film *film, int rank, int nranks, int image_layout, float min_voxel)
{
        if (s && need_device(s))
                return VRT_E_NODEVICE;
        if (!s || !ptrs)
                return fail(VRT_E_INVALID, "null argument");
        if (!fp->may_probe)
                if (int rc = no_probe_scene(s, fp->what))
                        return rc;
        if (has_light)
                if (int rc = film_ok(light_film))
                        return rc;
        if (int rc = film_ok(film))
                return rc;
        if (nranks < 1 || rank < 0 || rank >= nranks)
                return fail(VRT_E_INVALID, "rank %d of %d", rank, nranks);
        if (image_layout && nranks != 1)
                return fail(VRT_E_INVALID, "image_layout requires nranks == 1");
        if (int rc = trace_ok(s, min_voxel))
                return rc;
        fp->probe = !s->probes.empty();
        if (fp->probe)
                return device_expf(fp->what, &fp->fused);
        return VRT_OK;
}

static hipError_t frame_prim(vrt_scene *s, int set, const TraceParams &tp, const FramePath &fp, hipStream_t st)
{
        const hipError_t e = launch_trace_prim(tp, st, fp.probe ? &s->pdev : nullptr);
        if (e == hipSuccess)
                steps_commit(s, set, tp);
        return e;
}

static hipError_t frame_cones(vrt_scene *s, const TraceParams &tp, const FramePath &fp, hipStream_t st)
{
        return launch_cones(tp, st, fp.probe ? s->d_sgs : nullptr, fp.fused);
}

// A view over the latest light map on stream st, between the scene's timing
// events (caller holds s->mu, the device is set, a light map exists): the
// set is taken, the primary march and the cones + film pass are enqueued, and
// the set is released -- after a failure too, as batch_enqueue does.  d_hit /
// d_rgb: the per-sample outputs or null.
static int view_enqueue(vrt_scene *s, const FramePath &fp, const vrt_camera *cam, const vrt_film *film,
                        float min_voxel, int rank, int nranks, int image_layout, float *d_out, int32_t *d_hit,
                        float *d_rgb, hipStream_t st)
{
        const int set = s->lm_cur;  // the latest light map
        TraceParams tp0, tp;
        fill_trace_params(s, set, cam, film, min_voxel, rank, nranks, &tp0);
        tp0.r.image_layout = image_layout;
        tp0.r.out = d_out;
        tp0.r.so.hit = d_hit;
        tp0.r.so.rgb = d_rgb;
        if (int rc = trace_scratch(s, set, tp0, &tp))
                return rc;
        if (int rc = ts_acquire(s, set, st))
                return rc;
        hipError_t e = hipEventRecord(s->ev0, st);
        if (e == hipSuccess)
                e = frame_prim(s, set, tp, fp, st);
        if (e == hipSuccess)
                e = frame_cones(s, tp, fp, st);
        if (e == hipSuccess)
                e = hipEventRecord(s->ev1, st);
        if (e != hipSuccess) {
                (void)ts_release(s, set, st);
                return fail(VRT_E_DEVICE, "trace frame launch failed: %s", hipGetErrorString(e));
        }
        if (int rc = ts_release(s, set, st))
                return rc;
        s->timed = true;
        return VRT_OK;
}

static int render_trace_device(vrt_scene *s, FramePath fp, const vrt_camera *cam, const vrt_film *film,
                               float min_voxel, int rank, int nranks, int image_layout, float *d_out, void *stream)
{
        if (int rc = frame_args_ok(s, &fp, cam && d_out, false, nullptr, film, rank, nranks, image_layout, min_voxel))
                return rc;
        std::lock_guard<std::mutex> lk(s->mu);
        if (s->lm_cur < 0)
                return fail(VRT_E_INVALID, "no light map: call vrt_lightmap_build first");
        HIPCHK(hipSetDevice(s->device));
        return view_enqueue(s, fp, cam, film, min_voxel, rank, nranks, image_layout, d_out, nullptr, nullptr,
                            static_cast<hipStream_t>(stream));
}

static int render_trace_host(vrt_scene *s, FramePath fp, const vrt_camera *cam, const vrt_film *film,
                             float min_voxel, float *rgb, int32_t *s_hit, float *s_rgb)
{
        if (int rc = frame_args_ok(s, &fp, cam && rgb, false, nullptr, film, 0, 1, 1, min_voxel))
                return rc;
        std::lock_guard<std::mutex> lk(s->mu);
        if (s->lm_cur < 0)
                return fail(VRT_E_INVALID, "no light map: call vrt_lightmap_build first");
        HIPCHK(hipSetDevice(s->device));
        const size_t npix = (size_t)film->nx * film->ny, ns = npix * 4;
        DevMem img, dh, dr;
        HIPCHK(img.alloc(npix * 12));
        HIPCHK(hipMemsetAsync(img, 0, npix * 12, s->stream));
        if (s_hit) {
                HIPCHK(dh.alloc(ns * 4));
                HIPCHK(hipMemsetAsync(dh, 0, ns * 4, s->stream));
        }
        if (s_rgb) {
                HIPCHK(dr.alloc(ns * 12));
                HIPCHK(hipMemsetAsync(dr, 0, ns * 12, s->stream));
        }
        if (int rc = view_enqueue(s, fp, cam, film, min_voxel, 0, 1, 1, img.as<float>(),
                                  dh.as<int32_t>(), dr.as<float>(), s->stream))
                return rc;
        HIPCHK(hipStreamSynchronize(s->stream));
        HIPCHK(hipMemcpy(rgb, img, npix * 12, hipMemcpyDeviceToHost));
        if (s_hit)
                HIPCHK(hipMemcpy(s_hit, dh, ns * 4, hipMemcpyDeviceToHost));
        if (s_rgb)
                HIPCHK(hipMemcpy(s_rgb, dr, ns * 12, hipMemcpyDeviceToHost));
        return VRT_OK;
}

// The reference main() frame in one call (VRT/main.cc:75-126; on a probe
// scene with its probe block, :104-105, in place): light pass + filter on the
// scene's stream and, beside them on `stream`, the view's primary march (it
// reads neither the light map nor the SGs); with a light colour a probe
// scene's probes then gather behind the filter, on the scene's stream, into
// the device SGs; the cones + film pass waits for whichever came last.  Same
// values as vrt_lightmap_build followed by vrt_render_trace_device.  Returns
// once the filter is enqueued (the light pass's hit count needs one host
// sync); the image is ordered on `stream`.  The gather's records follow the
// view's in the set's block, and the gather builds the step table (the
// primary march does not read it).
//
// In three steps, for the single-scene calls (one after the other) and the
// multi-device handle (each step on every rank before the next), so the ranks'
// light passes do not queue behind each other's host sync:
//   frame_begin   the light march of the job's share of the light film and,
//                 beside it, the view's primary march;
//   frame_wait    the mid-build sync: the rank's hit count and its lists;
//   frame_finish  sort + sums + filter over `total` hits, the optional probe
//                 gather, the cones + film pass.
// A job without a view camera (the handle's light-map build, or a view with no
// tile) is the light-map build alone.  The job holds s->mu from frame_begin to
// frame_finish / frame_abort, which free it.
struct vrt::FrameJob {
        vrt_scene *s = nullptr;
        std::unique_lock<std::mutex> lk;
        FramePath fp{ "", true };
        bool view = false, gather = false;
        bool started = false;  // something is enqueued: a failure takes the bail path
        int set = 0;
        hipStream_t st = nullptr;
        float min_voxel = 0.f;
        float light[3] = {};
        size_t view_slots = 0;
        TraceParams tp;
        LightBuild lb;
};

// whatever was enqueued on either stream (the light pass and the gather on
// the scene's, the primary march on the caller's) finishes before the set's
// next user starts
static int frame_bail(FrameJob *j, int rc)
{
        vrt_scene *s = j->s;
        if (j->started && j->view) {
                if (hipEventRecord(s->lm_ev, s->stream) == hipSuccess)
                        (void)hipStreamWaitEvent(j->st, s->lm_ev, 0);
                (void)ts_release(s, j->set, j->st);
        }
        delete j;
        return rc;
}

int vrt::frame_check(vrt_scene *s, const FrameArgs &a)
{
        // without a light film: the view over the current light map alone
        FramePath fp{ a.what, true };
        if (a.nlights > 0 || a.lights) {
                if (int rc = frame_args_ok(s, &fp, a.cam && a.lights, false, nullptr, a.film, a.rank, a.nranks,
                                           a.image_layout, a.min_voxel))
                        return rc;
                return lights_ok(a.lights, a.nlights);
        }
        const bool has_light = a.light_film != nullptr;
        return frame_args_ok(s, &fp, a.cam && (a.light_cam || !has_light), has_light, a.light_film, a.film, a.rank,
                             a.nranks, a.image_layout, a.min_voxel);
}

int vrt::frame_begin(vrt_scene *s, const FrameArgs &a, FrameJob **out)
{
        *out = nullptr;
        FramePath fp{ a.what, a.may_probe };
        const bool fused = a.nlights > 0 || a.lights;
        if (a.cam) {
                if (int rc = frame_args_ok(s, &fp, (fused ? a.lights != nullptr : a.light_cam != nullptr) && a.d_out,
                                           !fused, a.light_film, a.film, a.rank, a.nranks, a.image_layout, a.min_voxel))
                        return rc;
        } else {
                if (s && need_device(s))
                        return VRT_E_NODEVICE;
                if (!s || !(fused ? (const void *)a.lights : (const void *)a.light_cam))
                        return fail(VRT_E_INVALID, "null argument");
                if (!fused)
                        if (int rc = film_ok(a.light_film))
                                return rc;
        }
        if (fused)
                if (int rc = lights_ok(a.lights, a.nlights))
                        return rc;
        if (a.light_nranks < 1 || a.light_rank < 0 || a.light_rank >= a.light_nranks)
                return fail(VRT_E_INVALID, "light rank %d of %d", a.light_rank, a.light_nranks);
        std::unique_ptr<FrameJob> job(new (std::nothrow) FrameJob);
        if (!job)
                return fail(VRT_E_NOMEM, "frame job alloc");
        FrameJob *j = job.get();
        j->s = s;
        j->lk = std::unique_lock<std::mutex>(s->mu);
        j->fp = fp;
        j->view = a.cam != nullptr;
        j->st = a.stream;
        j->min_voxel = a.min_voxel;
        HIPCHK(hipSetDevice(s->device));
        if (j->view && !s->lm_ev)
                HIPCHK(s->lm_ev.create(hipEventDisableTiming));
        if (j->view && fp.probe && !s->sg_ev)
                HIPCHK(s->sg_ev.create(hipEventDisableTiming));
        j->gather = j->view && fp.probe && a.light_color != nullptr;
        if (j->gather)
                std::memcpy(j->light, a.light_color, sizeof j->light);
        // alternate sets: this frame's light pass waits only for the frame
        // before last (the set's previous user), so it runs beside the
        // previous frame's cone-traced shading
        const int set = j->set = s->ts_next;
        s->ts_next ^= 1;
        if (j->view) {
                if (int rc = ensure_lm(s, set))  // the trace parameters point into it
                        return rc;
                TraceParams tp0;
                fill_trace_params(s, set, a.cam, a.film, a.min_voxel, a.rank, a.nranks, &tp0);
                tp0.r.image_layout = a.image_layout;
                tp0.r.out = a.d_out;
                // the view's records first, then (gather) one chunk of the gather's
                const int64_t nprobe = (int64_t)s->probes.size();
                j->view_slots = (size_t)tp0.r.tiles_this_rank * 256;
                const size_t gather_slots =
                        j->gather ? (size_t)std::min(nprobe, probe_chunk(100)) * kProbeSGs * 100 : 0;
                if (int rc = trace_scratch_n(s, set, tp0, j->view_slots + gather_slots, &j->tp))
                        return rc;
                if (j->gather)
                        j->tp.build_steps = 0;  // the gather builds the table, on the scene's stream
        }
        j->started = true;
        job.release();
        const vrt_light one = fused ? vrt_light{} : white_light(a.light_cam, a.light_film);
        if (int rc = light_begin(s, set, fused ? a.lights : &one, fused ? a.nlights : 1, fused, a.light_rank,
                                 a.light_nranks, &j->lb))
                return frame_bail(j, rc);
        if (j->view) {
                // the view's primary march beside the light pass (its records
                // wait only for the previous frame's users of the scratch)
                if (int rc = ts_acquire(s, set, j->st))
                        return frame_bail(j, rc);
                if (hipError_t e = frame_prim(s, set, j->tp, j->fp, j->st))
                        return frame_bail(j, fail(VRT_E_DEVICE, "primary march launch failed: %s", hipGetErrorString(e)));
        }
        *out = j;
        return VRT_OK;
}

int vrt::frame_wait(FrameJob *j, LightList *l)
{
        vrt_scene *s = j->s;
        if (hipSetDevice(s->device) != hipSuccess)
                return frame_bail(j, fail(VRT_E_DEVICE, "hipSetDevice failed"));
        if (int rc = light_wait(s, &j->lb))
                return frame_bail(j, rc);
        if (l) {
                l->keys = j->lb.k_in;
                l->samp = j->lb.samp;
                l->n = j->lb.nhit;
                l->cap = (uint64_t)j->lb.ns;
                l->stream = s->stream;
        }
        return VRT_OK;
}

int vrt::frame_finish(FrameJob *j, unsigned int total, bool merged)
{
        vrt_scene *s = j->s;
        const int set = j->set;
        if (hipSetDevice(s->device) != hipSuccess)
                return frame_bail(j, fail(VRT_E_DEVICE, "hipSetDevice failed"));
        if (int rc = light_finish(s, &j->lb, total, merged, j->view ? s->lm_ev.get() : nullptr))
                return frame_bail(j, rc);
        if (!j->view) {
                const int rc = ts_release(s, set, s->stream);
                delete j;
                return rc;
        }
        hipEvent_t last = s->lm_ev;  // what the cones + film pass waits for
        if (j->gather) {
                ProbeIO io{};
                io.probes = reinterpret_cast<const float *>(s->pdev.probes);
                io.n = (int64_t)s->probes.size();
                io.npoints = 100;
                std::memcpy(io.light, j->light, sizeof io.light);
                io.sgs = s->d_sgs;
                // the other set's last user may still read the device SGs
                if (int rc = ts_acquire(s, set ^ 1, s->stream))
                        return frame_bail(j, rc);
                s->sgs_stale = true;
                if (int rc = probe_enqueue(s, io, probe_default_points(), j->min_voxel, s->stream, j->view_slots))
                        return frame_bail(j, rc);
                last = s->sg_ev;
                if (hipError_t e = hipEventRecord(last, s->stream))
                        return frame_bail(j, fail(VRT_E_DEVICE, "hipEventRecord failed: %s", hipGetErrorString(e)));
        }
        hipError_t e = hipStreamWaitEvent(j->st, last, 0);
        if (e == hipSuccess)
                e = frame_cones(s, j->tp, j->fp, j->st);
        if (e != hipSuccess)
                return frame_bail(j, fail(VRT_E_DEVICE, "cone pass launch failed: %s", hipGetErrorString(e)));
        const int rc = ts_release(s, set, j->st);
        delete j;
        return rc;
}

void vrt::frame_abort(FrameJob *j)
{
        if (j) {
                (void)hipSetDevice(j->s->device);
                (void)frame_bail(j, VRT_OK);
        }
}

bool vrt::scene_has_lightmap(vrt_scene *s)
{
        std::lock_guard<std::mutex> lk(s->mu);
        return s->lm_cur >= 0;
}

int vrt::scene_stream_sync(vrt_scene *s)
{
        std::lock_guard<std::mutex> lk(s->mu);
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(hipStreamSynchronize(s->stream));
        return VRT_OK;
}

static int trace_frame_device(vrt_scene *s, FramePath fp, const vrt_camera *light_cam, const vrt_film *light_film,
                              const float *light_color, const vrt_camera *cam, const vrt_film *film,
                              float min_voxel, int rank, int nranks, int image_layout, float *d_out, void *stream,
                              int64_t *hits)
{
        if (!cam)  // a job without a view is the handle's; here a null argument
                return frame_args_ok(s, &fp, false, true, light_film, film, rank, nranks, image_layout, min_voxel);
        FrameArgs a{};
        a.what = fp.what;
        a.may_probe = fp.may_probe;
        a.light_cam = light_cam;
        a.light_film = light_film;
        a.light_color = light_color;
        a.light_rank = 0;
        a.light_nranks = 1;
        a.cam = cam;
        a.film = film;
        a.min_voxel = min_voxel;
        a.rank = rank;
        a.nranks = nranks;
        a.image_layout = image_layout;
        a.d_out = d_out;
        a.stream = static_cast<hipStream_t>(stream);
        FrameJob *j = nullptr;
        if (int rc = frame_begin(s, a, &j))
                return rc;
        LightList l{};
        if (int rc = frame_wait(j, &l))
                return rc;
        if (int rc = frame_finish(j, l.n, false))
                return rc;
        if (hits)
                *hits = (int64_t)l.n;
        return VRT_OK;
}

extern "C" int vrt_render_trace_device(vrt_scene *s, const vrt_camera *cam, const vrt_film *film,
                                       float min_voxel, int rank, int nranks, int image_layout,
                                       float *d_out, void *stream)
{
        return render_trace_device(s, { "vrt_render_trace_device", false }, cam, film, min_voxel, rank, nranks,
                                   image_layout, d_out, stream);
}

extern "C" int vrt_render_trace_probes_device(vrt_scene *s, const vrt_camera *cam, const vrt_film *film,
                                              float min_voxel, int rank, int nranks, int image_layout, float *d_out,
                                              void *stream)
{
        return render_trace_device(s, { "vrt_render_trace_probes_device", true }, cam, film, min_voxel, rank, nranks,
                                   image_layout, d_out, stream);
}

extern "C" int vrt_render_trace(vrt_scene *s, const vrt_camera *cam, const vrt_film *film, float min_voxel,
                                float *rgb, int32_t *s_hit, float *s_rgb)
{
        return render_trace_host(s, { "vrt_render_trace", false }, cam, film, min_voxel, rgb, s_hit, s_rgb);
}

extern "C" int vrt_render_trace_probes(vrt_scene *s, const vrt_camera *cam, const vrt_film *film, float min_voxel,
                                       float *rgb, int32_t *s_hit, float *s_rgb)
{
        return render_trace_host(s, { "vrt_render_trace_probes", true }, cam, film, min_voxel, rgb, s_hit, s_rgb);
}

extern "C" int vrt_trace_frame_device(vrt_scene *s, const vrt_camera *light_cam, const vrt_film *light_film,
                                      const vrt_camera *cam, const vrt_film *film, float min_voxel, int rank,
                                      int nranks, int image_layout, float *d_out, void *stream, int64_t *hits)
{
        return trace_frame_device(s, { "vrt_trace_frame_device", false }, light_cam, light_film, nullptr, cam, film,
                                  min_voxel, rank, nranks, image_layout, d_out, stream, hits);
}

extern "C" int vrt_trace_frame_probes_device(vrt_scene *s, const vrt_camera *light_cam,
                                             const vrt_film *light_film, const float *light_color,
                                             const vrt_camera *cam, const vrt_film *film, float min_voxel, int rank,
                                             int nranks, int image_layout, float *d_out, void *stream, int64_t *hits)
{
        return trace_frame_device(s, { "vrt_trace_frame_probes_device", true }, light_cam, light_film, light_color,
                                  cam, film, min_voxel, rank, nranks, image_layout, d_out, stream, hits);
}

extern "C" int vrt_trace_frame_lights_device(vrt_scene *s, const vrt_light *lights, int nlights,
                                             const float *probe_light_color, const vrt_camera *cam,
                                             const vrt_film *film, float min_voxel, int rank, int nranks,
                                             int image_layout, float *d_out, void *stream, int64_t *hits)
{
        FrameArgs a{};
        a.what = "vrt_trace_frame_lights_device";
        a.may_probe = true;
        a.lights = lights;
        a.nlights = nlights;
        a.light_color = probe_light_color;
        a.light_rank = 0;
        a.light_nranks = 1;
        a.cam = cam;
        a.film = film;
        a.min_voxel = min_voxel;
        a.rank = rank;
        a.nranks = nranks;
        a.image_layout = image_layout;
        a.d_out = d_out;
        a.stream = static_cast<hipStream_t>(stream);
        if (!cam || !lights || nlights < 1) {  // a job without a view is the handle's; here a bad argument
                if (s && need_device(s))
                        return VRT_E_NODEVICE;
                if (!s || !cam || !lights)
                        return fail(VRT_E_INVALID, "null argument");
                return lights_ok(lights, nlights);
        }
        FrameJob *j = nullptr;
        if (int rc = frame_begin(s, a, &j))
                return rc;
        LightList l{};
        if (int rc = frame_wait(j, &l))
                return rc;
        if (int rc = frame_finish(j, l.n, false))
                return rc;
        if (hits)
                *hits = (int64_t)l.n;
        return VRT_OK;
}

extern "C" int vrt_device_selftest(int device, const double *mt_in,
                                   double *mt_out, const float *sat_in,
                                   int32_t *sat_out, int64_t n)
{
        if (n < 0 || (mt_in && !mt_out) || (sat_in && !sat_out))
                return fail(VRT_E_INVALID, "bad argument");
        if (int rc = check_device(device))
                return rc;
        HIPCHK(hipSetDevice(device));
        DevMem a, b, c, d;
        if (mt_in) {
                HIPCHK(a.alloc((size_t)n * 15 * 8));
                HIPCHK(b.alloc((size_t)n * 4 * 8));
                HIPCHK(hipMemcpy(a, mt_in, (size_t)n * 15 * 8, hipMemcpyHostToDevice));
        }
        if (sat_in) {
                HIPCHK(c.alloc((size_t)n * 15 * 4));
                HIPCHK(d.alloc((size_t)n * 4));
                HIPCHK(hipMemcpy(c, sat_in, (size_t)n * 15 * 4, hipMemcpyHostToDevice));
        }
        HIPCHK(launch_selftest(a.as<double>(), b.as<double>(),
                               c.as<float>(), d.as<int32_t>(), n, nullptr));
        HIPCHK(hipDeviceSynchronize());
        if (mt_in)
                HIPCHK(hipMemcpy(mt_out, b, (size_t)n * 4 * 8, hipMemcpyDeviceToHost));
        if (sat_in)
                HIPCHK(hipMemcpy(sat_out, d, (size_t)n * 4, hipMemcpyDeviceToHost));
        return VRT_OK;
}

extern "C" int vrt_device_selftest_chain(int device, const float *cases, int64_t n, uint32_t *out)
{
        if (n < 0 || (n > 0 && (!cases || !out)))
                return fail(VRT_E_INVALID, "bad argument");
        if (int rc = check_device(device))
                return rc;
        if (n == 0)
                return VRT_OK;
        HIPCHK(hipSetDevice(device));
        DevMem din, dout;
        HIPCHK(din.alloc((size_t)n * 21 * sizeof(float)));
        HIPCHK(dout.alloc((size_t)n * 6 * sizeof(uint32_t)));
        HIPCHK(hipMemcpy(din, cases, (size_t)n * 21 * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(launch_selftest_chain(din.as<float>(), n, dout.as<uint32_t>(), nullptr));
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(out, dout, (size_t)n * 6 * sizeof(uint32_t), hipMemcpyDeviceToHost));
        return VRT_OK;
}

extern "C" int vrt_scene_chain_spacing(const vrt_scene *s, float out[3])
{
        if (!s || !out)
                return fail(VRT_E_INVALID, "null argument");
        for (int k = 0; k < 3; ++k)
                out[k] = s->ord_wmin[k];
        return VRT_OK;
}

extern "C" int vrt_device_selftest_order(int device, const float *dist, const uint32_t *hit_mask, int64_t n,
                                         uint32_t *orders, const float *depth, const int32_t *len, int64_t m,
                                         int32_t stride, int32_t *argmin)
{
        if (n < 0 || m < 0 || (n > 0 && (!dist || !hit_mask || !orders)) ||
            (m > 0 && (!depth || !len || !argmin || stride < 0)))
                return fail(VRT_E_INVALID, "bad argument");
        for (int64_t j = 0; j < m; ++j)
                if (len[j] < 0 || len[j] > stride)
                        return fail(VRT_E_INVALID, "record list %lld: length %d outside [0, %d]", (long long)j,
                                    len[j], stride);
        if (int rc = check_device(device))
                return rc;
        HIPCHK(hipSetDevice(device));
        DevMem dd, dh, dout, ddep, dlen, darg;
        if (n > 0) {
                HIPCHK(dd.alloc((size_t)n * 8 * sizeof(float)));
                HIPCHK(dh.alloc((size_t)n * sizeof(uint32_t)));
                HIPCHK(dout.alloc((size_t)n * 6 * sizeof(uint32_t)));
                HIPCHK(hipMemcpy(dd, dist, (size_t)n * 8 * sizeof(float), hipMemcpyHostToDevice));
                HIPCHK(hipMemcpy(dh, hit_mask, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
        if (m > 0) {
                HIPCHK(ddep.alloc(std::max<size_t>(1, (size_t)m * stride) * sizeof(float)));
                HIPCHK(dlen.alloc((size_t)m * sizeof(int32_t)));
                HIPCHK(darg.alloc((size_t)m * sizeof(int32_t)));
                if (stride > 0)
                        HIPCHK(hipMemcpy(ddep, depth, (size_t)m * stride * sizeof(float), hipMemcpyHostToDevice));
                HIPCHK(hipMemcpy(dlen, len, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice));
        }
        HIPCHK(launch_selftest_order(dd.as<float>(), dh.as<uint32_t>(), n,
                                     dout.as<uint32_t>(), ddep.as<float>(),
                                     dlen.as<int32_t>(), m, stride, darg.as<int32_t>(),
                                     nullptr));
        HIPCHK(hipDeviceSynchronize());
        if (n > 0)
                HIPCHK(hipMemcpy(orders, dout, (size_t)n * 6 * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (m > 0)
                HIPCHK(hipMemcpy(argmin, darg, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
        return VRT_OK;
}

// ---------------------------------------------------------------------------
// scene update (vrt_scene_update, vrt_scene_update_device): new vertex
// positions (and normals) on the live handle.  A device scene rebuilds on the
// GPU -- root box, frontier build, then the finish kernels of vrt_build.hip
// (leaf records, per-record boxes, march records, chain spacing, TriPos /
// TriAttr) -- and copies back only what host code reads (nodes, node_vox,
// ref_tri).  Everything that can refuse happens before the first write to an
// array the scene is using, so a refused update leaves the scene as it was.
// A scene with light probes moves through vrt_scene_update_probes[_device],
// the same path with the probes in the root box and in the frontier build.
// ---------------------------------------------------------------------------
// probe_call: vrt_scene_update_probes[_device], which takes the scenes with
// light probes that vrt_scene_update refuses, and no others
// for_handle: the call is vrt_multi_update's, which moves every rank alike
static int update_args_ok(vrt_scene *s, const float *pos, const char *what, bool probe_call = false,
                          bool for_handle = false)
{
        if (!s || !pos)
                return fail(VRT_E_INVALID, "%s: null argument", what);
        if (probe_call && s->probes.empty())
                return fail(VRT_E_INVALID, "%s: the scene has no light probes; use vrt_scene_update", what);
        if (!probe_call)
                if (int rc = no_probe_scene(s, what))
                        return rc;
        if (s->owned && !for_handle)
                return fail(VRT_E_INVALID, "%s: the scene is a rank of a vrt_multi handle, whose ranks must stay replicas",
                            what);
        if ((uint32_t)s->ntri > 0x55555555u)
                return fail(VRT_E_INVALID, "%s: %d triangles, 3 x that must stay below 2^32", what, s->ntri);
        // the root box's sequence numbers: the vertices, then the probes
        if (3ull * (uint64_t)s->ntri + (uint64_t)s->probes.size() > 0x100000000ull)
                return fail(VRT_E_INVALID, "%s: 3 x %d triangles + %zu probes must stay within 2^32", what, s->ntri,
                            s->probes.size());
        return VRT_OK;
}

// The host-only scene: the host build and finish on the new arrays, made
// beside the scene and swapped in.
static int update_host(vrt_scene *s, const float *pos, const float *nrm, const vrt_probe *probes)
{
        const double t0 = now_ms();
        std::unique_ptr<vrt_scene> t(new (std::nothrow) vrt_scene);
        if (!t)
                return fail(VRT_E_NOMEM, "scene alloc");
        t->device = -1;
        t->max_depth = s->max_depth;
        t->ntri = s->ntri;
        vrt_scene_desc d{};
        d.ntri = s->ntri;
        d.pos = pos;
        d.nrm = nrm;
        try {
                // a probe scene: the new probes, or the ones it has
                if (probes)
                        t->probes.assign(probes, probes + s->probes.size());
                else
                        t->probes = s->probes;
                if (int rc = build_tree(t.get(), &d, false))
                        return rc;
                const int n = s->ntri;
                t->tri_pos.resize((size_t)n);
                t->tri_attr = s->tri_attr;  // uvs, materials and, without nrm, the normals stay
                for (int i = 0; i < n; ++i) {
                        TriPos &tp = t->tri_pos[i];
                        std::memcpy(tp.p, pos + 9 * (size_t)i, sizeof tp.p);
                        tp.pad[0] = tp.pad[1] = tp.pad[2] = 0.f;
                        if (!nrm)
                                continue;
                        TriAttr &ta = t->tri_attr[i];
                        for (int v = 0; v < 3; ++v) {
                                const float *nn = nrm + 9 * (size_t)i + 3 * v;
                                const f3 q = normalize(mk3(nn[0], nn[1], nn[2]));
                                ta.n[3 * v + 0] = q.x;
                                ta.n[3 * v + 1] = q.y;
                                ta.n[3 * v + 2] = q.z;
                        }
                }
        } catch (const std::bad_alloc &) {
                return fail(VRT_E_NOMEM, "scene update: out of host memory");
        }
        s->nodes.swap(t->nodes);
        s->node_vox.swap(t->node_vox);
        s->refs48.swap(t->refs48);
        s->refs64.swap(t->refs64);
        s->wide_leaves = t->wide_leaves;
        s->ref_tri.swap(t->ref_tri);
        s->tri_pos.swap(t->tri_pos);
        s->tri_attr.swap(t->tri_attr);
        s->level_begin.swap(t->level_begin);
        s->probes.swap(t->probes);
        s->pnode.swap(t->pnode);
        s->pref.swap(t->pref);
        s->probe_leaves = t->probe_leaves;
        s->info.nodes = t->info.nodes;
        s->info.internal = t->info.internal;
        s->info.leaves = t->info.leaves;
        s->info.nonempty_leaves = t->info.nonempty_leaves;
        s->info.tri_refs = t->info.tri_refs;
        for (int k = 0; k < 3; ++k) {
                s->info.root_min[k] = t->info.root_min[k];
                s->info.root_max[k] = t->info.root_max[k];
        }
        s->info.build_ms = now_ms() - t0;
        s->info.build_device_ms = 0;
        s->up_ms[0] = s->up_ms[3] = s->info.build_ms;
        s->up_ms[1] = s->up_ms[2] = 0;
        s->updated = true;
        return VRT_OK;
}

// async copy to the host in the stream's order
static hipError_t fetch(void *dst, const void *src, size_t bytes, hipStream_t st)
{
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
}

// pos / nrm / probes: host arrays (on_device false: copied to the scratch
// first) or device arrays read in the order of the caller's stream cst.  A
// probe scene (vrt_scene_update_probes; probes == nullptr: they stay) adds the
// probes' faces to the root box, the probe frontier to the build, and pnode /
// pref / the probes to what is swapped in and copied back.
//
// The update's first half: everything that can refuse.  It writes only the
// scene's BuildScratch and memory the scene does not read yet (plan->grown,
// the spare host mirrors), so that a plan which is dropped leaves the scene
// as it was.
int vrt::update_prepare(vrt_scene *s, const float *pos, const float *nrm, const vrt_probe *probes, bool on_device,
                        hipStream_t cst, bool fail_limit, UpdatePlan *plan)
{
        UpdatePlan &pl = *plan;
        pl.t0 = now_ms();
        // Wait for all work the scene has in flight.  Not every launch leaves
        // an event to wait for: a grid-kind render (every 64-B-record scene)
        // and the device ray-march batches run on the caller's stream and
        // record none.  So the whole device is waited for, which covers every
        // stream a kernel that reads the scene's arrays can be on.
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(hipDeviceSynchronize());
        hipStream_t st = s->stream;
        if (!s->up_e0) {
                HIPCHK(s->up_in.create(hipEventDisableTiming));
                HIPCHK(s->up_e0.create());
                HIPCHK(s->up_e1.create());
        }
        BuildScratch &sc = s->bscratch;
        const int n = s->ntri;
        const int np = (int)s->probes.size();
        const float *d_pos = pos, *d_nrm = nrm;
        // the probes the build reads: the caller's, or the scene's own
        const float4 *d_probes = np ? s->pdev.probes : nullptr;
        if (on_device) {
                HIPCHK(hipEventRecord(s->up_in, cst));
                HIPCHK(hipStreamWaitEvent(st, s->up_in, 0));
                if (np && probes) {
                        d_probes = reinterpret_cast<const float4 *>(probes);
                        // vrt_probe promises 4-byte alignment (a slice of a larger
                        // array); the kernels load float4, so such an array goes
                        // through the scratch copy a host array takes
                        if (reinterpret_cast<uintptr_t>(probes) % sizeof(float4)) {
                                HIPCHK(sc.probes.need((size_t)np * sizeof(float4)));
                                HIPCHK(hipMemcpyAsync(sc.probes, probes, (size_t)np * sizeof(float4),
                                                      hipMemcpyDeviceToDevice, st));
                                d_probes = sc.probes.as<float4>();
                        }
                }
        } else {
                HIPCHK(sc.pos.need((size_t)n * 36));
                HIPCHK(hipMemcpyAsync(sc.pos, pos, (size_t)n * 36, hipMemcpyHostToDevice, st));
                d_pos = sc.pos.as<float>();
                if (nrm) {
                        HIPCHK(sc.nrm.need((size_t)n * 36));
                        HIPCHK(hipMemcpyAsync(sc.nrm, nrm, (size_t)n * 36, hipMemcpyHostToDevice, st));
                        d_nrm = sc.nrm.as<float>();
                }
                if (np && probes) {
                        HIPCHK(sc.probes.need((size_t)np * sizeof(float4)));
                        HIPCHK(hipMemcpyAsync(sc.probes, probes, (size_t)np * sizeof(float4), hipMemcpyHostToDevice, st));
                        d_probes = sc.probes.as<float4>();
                }
        }
        const bool new_probes = np && probes;
        pl.d_pos = d_pos;
        pl.d_nrm = d_nrm;
        pl.d_probes = d_probes;
        pl.new_probes = new_probes;
        HIPCHK(hipEventRecord(s->up_e0, st));
        // root box: 6 keys, then the 6 floats the host needs for info and, on a
        // probe scene, the index of the first probe creation would refuse
        float *const root = pl.root;
        uint32_t bad_probe = 0xFFFFFFFFu;
        HIPCHK(sc.root.need(128));
        HIPCHK(launch_root_box(d_pos, n, d_probes, np, sc.root.as<uint64_t>(), sc.root.as<float>() + 12, st));
        HIPCHK(fetch(root, sc.root.as<float>() + 12, (np ? 7 : 6) * sizeof(float), st));
        HIPCHK(hipStreamSynchronize(st));
        if (np)
                std::memcpy(&bad_probe, &root[6], sizeof bad_probe);
        if (new_probes && bad_probe != 0xFFFFFFFFu)
                return fail(VRT_E_INVALID, "probe %u: centre must be finite, radius finite and >= 0", bad_probe);
        DeviceTree &tree = pl.tree;
        try {
                std::string err;
                if (build_frontier_device(sc, d_pos, n, root, root + 3, s->max_depth, d_probes, np, st, fail_limit,
                                          &tree, &err) != hipSuccess) {
                        (void)hipGetLastError();
                        (void)hipStreamSynchronize(st);
                        if (tree.too_large)
                                return fail(VRT_E_INVALID, "%s", err.c_str());
                        return fail(VRT_E_DEVICE, "device octree build: %s", err.c_str());
                }
        } catch (const std::bad_alloc &) {
                // the build's host vectors; it has written only its own scratch
                (void)hipStreamSynchronize(st);
                return fail(VRT_E_NOMEM, "scene update: out of host memory");
        }
        const int64_t nn = tree.nnodes, nr = tree.nrefs;
        unsigned int *const counts = pl.counts;
        HIPCHK(sc.counts.need(16));
        HIPCHK(launch_leaf_counts(tree.nodes, nn, sc.counts.as<unsigned int>(), st));
        HIPCHK(fetch(counts, sc.counts, sizeof pl.counts, st));
        HIPCHK(hipStreamSynchronize(st));
        // the choices upload() makes, on the new geometry
        const bool wide = (size_t)nr >= 8 * (size_t)std::max<int64_t>(1, (int64_t)counts[1]);
        float ext = 0.f;
        bool fast = true;
        for (int k = 0; k < 3; ++k) {
                ext = std::max(ext, root[3 + k] - root[k]);
                fast = fast && std::fabs(root[k]) < 0x1p60f && std::fabs(root[3 + k]) < 0x1p60f;
        }
        const bool lb_on = ext > 0.f && std::isfinite(ext);
        const bool rboxes = VRT_LEAF_CULL && !wide && lb_on;
        const size_t refs_bytes = (size_t)nr * (wide ? sizeof(RefRec64) : sizeof(RefRec48));
        const size_t sz_rbox = rboxes ? align_up(((size_t)nr + kRefBoxPad) * sizeof(RefBox)) : 0;
        // a probe scene's pnode (one per node) and pref (one per probe
        // reference) as upload() sizes them; nothing on any other scene
        const int64_t npr = tree.nprefs;
        constexpr int kOwners = UpdatePlan::kOwners;
        const size_t want[kOwners] = { align_up((size_t)nn * sizeof(NodeRec)), align_up((size_t)nn * sizeof(uint32_t)),
                                       align_up(sz_rbox + std::max<size_t>(64, refs_bytes)),
                                       align_up((size_t)nn * sizeof(XNodeRec)),
                                       np ? align_up((size_t)nn * sizeof(uint2)) : 0,
                                       np ? align_up(std::max<size_t>(1, (size_t)npr) * sizeof(uint32_t)) : 0 };
        // larger arrays are made beside the ones in use and swapped in only
        // when all of them exist
        DevMem *const own[kOwners] = { &s->g_nodes, &s->g_vox, &s->g_refs, &s->g_xnodes, &s->g_pnode, &s->g_pref };
        DevMem *const grown = pl.grown;
        std::vector<NodeRec> &h_nodes = s->up_nodes;
        std::vector<uint32_t> &h_vox = s->up_vox, &h_reftri = s->up_ref_tri;
        for (int i = 0; i < kOwners; ++i)
                if (own[i]->size() < want[i] && grown[i].alloc(want[i]) != hipSuccess) {
                        (void)hipGetLastError();
                        return fail(VRT_E_DEVICE, "scene update: no device memory for %zu bytes", want[i]);
                }
        if (sc.ref_tri.need((size_t)nr * 4) != hipSuccess || sc.lohi.need(lb_on ? (size_t)nn * 48 : 0) != hipSuccess ||
            sc.chain.need(32) != hipSuccess) {
                (void)hipGetLastError();
                return fail(VRT_E_DEVICE, "scene update: no device memory for the finish scratch");
        }
        try {
                h_nodes.resize((size_t)nn);
                h_vox.resize((size_t)nn);
                h_reftri.resize((size_t)nr);
                if (np) {
                        s->up_pnode.resize((size_t)nn);
                        s->up_pref.resize((size_t)npr);
                        if (new_probes)
                                s->up_probes.resize((size_t)np);
                }
        } catch (const std::bad_alloc &) {
                return fail(VRT_E_NOMEM, "scene update: out of host memory");
        }
        pl.wide = wide;
        pl.fast = fast;
        pl.lb_on = lb_on;
        pl.rboxes = rboxes;
        pl.ext = ext;
        pl.sz_rbox = sz_rbox;
        return VRT_OK;
}

// The update's second half.
int vrt::update_commit(vrt_scene *s, UpdatePlan *plan)
{
        UpdatePlan &pl = *plan;
        constexpr int kOwners = UpdatePlan::kOwners;
        hipStream_t st = s->stream;
        BuildScratch &sc = s->bscratch;
        const int n = s->ntri;
        const int np = (int)s->probes.size();
        const float *const d_pos = pl.d_pos, *const d_nrm = pl.d_nrm;
        const float4 *const d_probes = pl.d_probes;
        const bool new_probes = pl.new_probes;
        const float *const root = pl.root;
        DeviceTree &tree = pl.tree;
        const int64_t nn = tree.nnodes, nr = tree.nrefs, npr = tree.nprefs;
        const unsigned int *const counts = pl.counts;
        const bool wide = pl.wide, fast = pl.fast, lb_on = pl.lb_on, rboxes = pl.rboxes;
        const float ext = pl.ext;
        const size_t sz_rbox = pl.sz_rbox;
        const double t0 = pl.t0;
        DevMem *const own[kOwners] = { &s->g_nodes, &s->g_vox, &s->g_refs, &s->g_xnodes, &s->g_pnode, &s->g_pref };
        DevMem *const grown = pl.grown;
        std::vector<NodeRec> &h_nodes = s->up_nodes;
        std::vector<uint32_t> &h_vox = s->up_vox, &h_reftri = s->up_ref_tri;
        HIPCHK(hipSetDevice(s->device));
        // ---- nothing below refuses: the scene's arrays are written from here
        // on.  The device pointers follow their owners at once, so that no
        // later error return leaves one on released memory (after a
        // VRT_E_DEVICE from here on the scene's contents are undefined).
        const size_t old_nodes = s->nodes.size();
        for (int i = 0; i < kOwners; ++i)
                if (grown[i])
                        *own[i] = std::move(grown[i]);
        s->wide_leaves = wide;
        s->rboxes = rboxes;
        s->dev.nodes = s->g_nodes.as<NodeRec>();
        s->dev.node_vox = s->g_vox.as<uint32_t>();
        s->dev.refs = s->g_refs.as<char>() + sz_rbox;
        s->dev.xnodes = s->g_xnodes.as<XNodeRec>();
        s->dev.wide_leaves = wide ? 1 : 0;
        HIPCHK(hipMemcpyAsync(s->g_nodes, tree.nodes, (size_t)nn * sizeof(NodeRec), hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(s->g_vox, tree.node_vox, (size_t)nn * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        if (np) {
                // the probes and the stored SGs keep their place in d_probe,
                // whose size never changes: only the probes' values move
                s->pdev.pnode = s->g_pnode.as<uint2>();
                s->pdev.pref = s->g_pref.as<uint32_t>();
                HIPCHK(hipMemcpyAsync(s->g_pnode, tree.pnode, (size_t)nn * sizeof(uint2), hipMemcpyDeviceToDevice, st));
                if (npr)
                        HIPCHK(hipMemcpyAsync(s->g_pref, tree.pref, (size_t)npr * sizeof(uint32_t),
                                              hipMemcpyDeviceToDevice, st));
                if (new_probes)
                        HIPCHK(hipMemcpyAsync(const_cast<float4 *>(s->pdev.probes), d_probes,
                                              (size_t)np * sizeof(float4), hipMemcpyDeviceToDevice, st));
        }
        FinishArgs fa{};
        fa.tree = &tree;
        fa.pos = d_pos;
        fa.nrm = d_nrm;
        fa.ntri = n;
        fa.wide = wide ? 1 : 0;
        fa.rboxes = rboxes ? 1 : 0;
        fa.lb_on = lb_on ? 1 : 0;
        fa.eps = std::ldexp((double)ext, -16);
        fa.chain = fast ? 1 : 0;
        fa.refs = s->g_refs.as<char>() + sz_rbox;
        fa.ref_tri = sc.ref_tri.as<uint32_t>();
        fa.xnodes = s->g_xnodes.as<XNodeRec>();
        fa.lohi = sc.lohi.as<double>();
        fa.chain_out = sc.chain.as<uint64_t>();
        fa.tri_pos = const_cast<TriPos *>(s->dev.tri_pos);
        fa.tri_attr = const_cast<TriAttr *>(s->dev.tri_attr);
        HIPCHK(launch_finish(fa, st));
        HIPCHK(hipEventRecord(s->up_e1, st));
        HIPCHK(hipEventSynchronize(s->up_e1));
        const double t1 = now_ms();
        uint64_t chain[4] = { ~0ull, ~0ull, ~0ull, 1 };
        HIPCHK(fetch(h_nodes.data(), tree.nodes, (size_t)nn * sizeof(NodeRec), st));
        HIPCHK(fetch(h_vox.data(), tree.node_vox, (size_t)nn * sizeof(uint32_t), st));
        HIPCHK(fetch(h_reftri.data(), fa.ref_tri, (size_t)nr * 4, st));
        if (fast)
                HIPCHK(fetch(chain, fa.chain_out, sizeof chain, st));
        unsigned int probe_leaves = 0;
        if (np) {
                HIPCHK(fetch(s->up_pnode.data(), tree.pnode, (size_t)nn * sizeof(uint2), st));
                HIPCHK(fetch(s->up_pref.data(), tree.pref, (size_t)npr * sizeof(uint32_t), st));
                if (tree.probe_leaves)
                        HIPCHK(fetch(&probe_leaves, tree.probe_leaves, sizeof probe_leaves, st));
                if (new_probes)
                        HIPCHK(fetch(s->up_probes.data(), d_probes, (size_t)np * sizeof(float4), st));
        }
        HIPCHK(hipStreamSynchronize(st));
        const double t2 = now_ms();
        // ---- host mirrors and the scene's constants
        s->nodes.swap(h_nodes);
        s->node_vox.swap(h_vox);
        s->ref_tri.swap(h_reftri);
        s->level_begin.swap(tree.level_begin);
        if (np) {
                s->pnode.swap(s->up_pnode);
                s->pref.swap(s->up_pref);
                s->probe_leaves = probe_leaves;
                if (new_probes)
                        s->probes.swap(s->up_probes);
        }
        // no reader after upload() on a scene that cannot be replicated
        std::vector<RefRec48>().swap(s->refs48);
        std::vector<RefRec64>().swap(s->refs64);
        std::vector<TriPos>().swap(s->tri_pos);
        std::vector<TriAttr>().swap(s->tri_attr);
        s->info.nodes = nn;
        s->info.internal = tree.ninternal;
        s->info.leaves = counts[0];
        s->info.nonempty_leaves = counts[1];
        s->info.tri_refs = nr;
        for (int k = 0; k < 3; ++k) {
                s->info.root_min[k] = root[k];
                s->info.root_max[k] = root[3 + k];
                s->dev.lb_center[k] = 0.5f * (root[k] + root[3 + k]);
        }
        s->dev.lb_reach = lb_on ? 16.f * ext : -1.f;
        s->dev.fast_ok = fast ? 1 : 0;
        // chain_spacing's tail on the reduced minima
        for (int k = 0; k < 3; ++k)
                s->ord_wmin[k] = 0.f;
        if (fast) {
                bool ok = chain[3] == 0;
                const bool any = tree.ninternal > 0;
                float f[3];
                for (int k = 0; k < 3; ++k) {
                        const double w = chain[k] == ~0ull ? HUGE_VAL : chain_key_value(chain[k]);
                        ok = ok && any && std::isfinite(w) && w > 0.0;
                        f[k] = (float)w;
                        if (ok && (double)f[k] > w)
                                f[k] = std::nextafter(f[k], 0.f);
                        ok = ok && f[k] > 0.f;
                }
                if (ok)
                        for (int k = 0; k < 3; ++k)
                                s->ord_wmin[k] = f[k];
        }
        int64_t bytes = (int64_t)(s->d_mem.size() + s->d_probe.size());
        for (int i = 0; i < kOwners; ++i)
                bytes += (int64_t)own[i]->size();
        s->info.device_bytes = bytes;
        // ---- derived state back to a fresh scene's; the allocations stay
        // where their size still fits
        for (TraceSet &t : s->ts) {
                t.steps_key[0] = t.steps_key[1] = -1.f;
                if (!t.lm)
                        continue;
                if (s->nodes.size() != old_nodes) {
                        t.lm.reset();  // sized by the node count: made again on first use
                        continue;
                }
                std::vector<float4> cells;
                try {
                        cells = cone_cells(s->nodes);
                } catch (const std::bad_alloc &) {
                        t.lm.reset();  // no host memory for the cells now: made again on first use
                        continue;
                }
                HIPCHK(hipMemcpy(t.lm.as<char>() + (size_t)nn * (sizeof(LMRec) + sizeof(float4)) + 256, cells.data(),
                                 cells.size() * sizeof(float4), hipMemcpyHostToDevice));
        }
        s->ts_next = 0;
        s->lm_cur = -1;
        for (int64_t &v : s->lm_stats)
                v = 0;
        s->timed = false;
        s->entry_slot = -1;
        s->entry_units = 0;
        s->spill_last = -1;
        s->spill_want = 0;
        s->spill_next = 0;
        float gpu_ms = 0.f;
        HIPCHK(hipEventElapsedTime(&gpu_ms, s->up_e0, s->up_e1));
        const double t3 = now_ms();
        s->up_ms[0] = t3 - t0;
        s->up_ms[1] = gpu_ms;
        s->up_ms[2] = t2 - t1;
        s->up_ms[3] = std::max(0.0, s->up_ms[0] - s->up_ms[1] - s->up_ms[2]);
        s->info.build_ms = s->up_ms[0];
        s->info.build_device_ms = gpu_ms;
        s->info.upload_ms = 0;
        s->updated = true;
        return VRT_OK;
}

// the single-scene entry points: the two halves back to back
static int update_device(vrt_scene *s, const float *pos, const float *nrm, const vrt_probe *probes, bool on_device,
                         hipStream_t cst)
{
        UpdatePlan plan;
        if (int rc = update_prepare(s, pos, nrm, probes, on_device, cst,
                                    (test_flags() & VRT_TEST_UPDATE_TOO_LARGE) != 0, &plan))
                return rc;
        return update_commit(s, &plan);
}

int vrt::update_probes_ok(const vrt_probe *probes, size_t n)
{
        for (size_t k = 0; k < n; ++k) {
                const vrt_probe &pb = probes[k];
                if (!std::isfinite(pb.o[0]) || !std::isfinite(pb.o[1]) || !std::isfinite(pb.o[2]) ||
                    !std::isfinite(pb.r) || pb.r < 0.f)
                        return fail(VRT_E_INVALID, "probe %zu: centre must be finite, radius finite and >= 0", k);
        }
        return VRT_OK;
}

// A rank scene of a vrt_multi handle, checked once for the handle's update:
// update_args_ok without the refusal of an owned scene, which is the handle's
// own to lift.
int vrt::update_multi_args_ok(vrt_scene *s, const float *pos, bool has_probes, const char *what)
{
        if (has_probes && s->probes.empty())
                return fail(VRT_E_INVALID, "%s: the handle has no light probes", what);
        return update_args_ok(s, pos, what, !s->probes.empty(), true);
}

int vrt::update_stage(vrt_scene *s, bool nrm, bool probes, float **d_pos, float **d_nrm, vrt_probe **d_probes,
                      size_t bytes[3])
{
        BuildScratch &sc = s->bscratch;
        bytes[0] = (size_t)s->ntri * 36;
        bytes[1] = nrm ? bytes[0] : 0;
        bytes[2] = probes ? s->probes.size() * sizeof(vrt_probe) : 0;
        // the scratch's last user (the previous update) returned with its work done
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(sc.pos.need(bytes[0]));
        *d_pos = sc.pos.as<float>();
        *d_nrm = nullptr;
        *d_probes = nullptr;
        if (nrm) {
                HIPCHK(sc.nrm.need(bytes[1]));
                *d_nrm = sc.nrm.as<float>();
        }
        if (probes) {
                HIPCHK(sc.probes.need(bytes[2]));
                *d_probes = sc.probes.as<vrt_probe>();
        }
        return VRT_OK;
}

std::mutex &vrt::scene_mutex(vrt_scene *s) { return s->mu; }

void vrt::scene_replica_key(const vrt_scene *s, int *wide, float wmin[3])
{
        *wide = s->wide_leaves ? 1 : 0;
        for (int k = 0; k < 3; ++k)
                wmin[k] = s->ord_wmin[k];
}

int vrt::scene_device(const vrt_scene *s) { return s->device; }

size_t vrt::scene_nprobe(const vrt_scene *s) { return s->probes.size(); }

int vrt::scene_test_flip_attr(vrt_scene *s)
{
        if (s->ntri < 1)
                return VRT_OK;
        std::lock_guard<std::mutex> lk(s->mu);
        HIPCHK(hipSetDevice(s->device));
        uint32_t w = 0;
        HIPCHK(hipMemcpy(&w, s->dev.tri_attr, sizeof w, hipMemcpyDeviceToHost));
        w ^= 1u;
        HIPCHK(hipMemcpy(const_cast<TriAttr *>(s->dev.tri_attr), &w, sizeof w, hipMemcpyHostToDevice));
        return VRT_OK;
}

extern "C" int vrt_scene_update(vrt_scene *s, const float *pos, const float *nrm)
{
        if (int rc = update_args_ok(s, pos, "vrt_scene_update"))
                return rc;
        std::lock_guard<std::mutex> lk(s->mu);
        if (!s->d_mem)
                return update_host(s, pos, nrm, nullptr);
        return update_device(s, pos, nrm, nullptr, false, nullptr);
}

extern "C" int vrt_scene_update_device(vrt_scene *s, const float *d_pos, const float *d_nrm, void *stream)
{
        if (s && need_device(s))
                return VRT_E_NODEVICE;
        if (int rc = update_args_ok(s, d_pos, "vrt_scene_update_device"))
                return rc;
        std::lock_guard<std::mutex> lk(s->mu);
        return update_device(s, d_pos, d_nrm, nullptr, true, static_cast<hipStream_t>(stream));
}

extern "C" int vrt_scene_update_probes(vrt_scene *s, const float *pos, const float *nrm, const vrt_probe *probes)
{
        if (int rc = update_args_ok(s, pos, "vrt_scene_update_probes", true))
                return rc;
        std::lock_guard<std::mutex> lk(s->mu);
        // as at creation; the device variant's check is the root-box kernel's
        if (probes)
                if (int rc = update_probes_ok(probes, s->probes.size()))
                        return rc;
        if (!s->d_mem)
                return update_host(s, pos, nrm, probes);
        return update_device(s, pos, nrm, probes, false, nullptr);
}

extern "C" int vrt_scene_update_probes_device(vrt_scene *s, const float *d_pos, const float *d_nrm,
                                              const vrt_probe *d_probes, void *stream)
{
        if (s && need_device(s))
                return VRT_E_NODEVICE;
        if (int rc = update_args_ok(s, d_pos, "vrt_scene_update_probes_device", true))
                return rc;
        std::lock_guard<std::mutex> lk(s->mu);
        return update_device(s, d_pos, d_nrm, d_probes, true, static_cast<hipStream_t>(stream));
}

extern "C" int vrt_scene_update_stats(const vrt_scene *s, double ms[4])
{
        if (!s || !ms)
                return fail(VRT_E_INVALID, "null argument");
        if (!s->updated)
                return fail(VRT_E_INVALID, "the scene has not been updated");
        for (int k = 0; k < 4; ++k)
                ms[k] = s->up_ms[k];
        return VRT_OK;
}

extern "C" int vrt_scene_update_scratch(vrt_scene *s, int release, int64_t *bytes)
{
        if (!s || !bytes)
                return fail(VRT_E_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(s->mu);
        *bytes = (int64_t)s->bscratch.bytes();
        if (!release || !s->d_mem)
                return VRT_OK;
        // an update returns with its work done: nothing is using the scratch
        HIPCHK(hipSetDevice(s->device));
        s->bscratch = BuildScratch();
        std::vector<NodeRec>().swap(s->up_nodes);
        std::vector<uint32_t>().swap(s->up_vox);
        std::vector<uint32_t>().swap(s->up_ref_tri);
        std::vector<uint2>().swap(s->up_pnode);
        std::vector<uint32_t>().swap(s->up_pref);
        std::vector<vrt_probe>().swap(s->up_probes);
        return VRT_OK;
}

extern "C" int vrt_scene_device_array(vrt_scene *s, int kind, void *out, int64_t cap, int64_t *bytes)
{
        if (s && need_device(s))
                return VRT_E_NODEVICE;
        if (!s || !bytes)
                return fail(VRT_E_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(s->mu);
        const size_t nr = s->ref_tri.size();
        const void *src = nullptr;
        size_t n = 0;
        const int last = s->probes.empty() ? 4 : 7;  // 5 to 7: a probe scene's side arrays
        if (kind < 0 || kind > last)
                return fail(VRT_E_INVALID, "vrt_scene_device_array: kind %d outside [0, %d]", kind, last);
        switch (kind) {
        case 0:
                src = s->dev.refs;
                n = nr * (s->wide_leaves ? sizeof(RefRec64) : sizeof(RefRec48));
                break;
        case 1:
                n = s->rboxes ? nr * sizeof(RefBox) : 0;
                src = static_cast<const char *>(s->dev.refs) - n;
                break;
        case 2:
                src = s->dev.xnodes;
                n = s->nodes.size() * sizeof(XNodeRec);
                break;
        case 3:
                src = s->dev.tri_pos;
                n = (size_t)s->ntri * sizeof(TriPos);
                break;
        case 4:
                src = s->dev.tri_attr;
                n = (size_t)s->ntri * sizeof(TriAttr);
                break;
        case 5:
                src = s->pdev.pnode;
                n = s->pnode.size() * sizeof(uint2);
                break;
        case 6:
                src = s->pdev.pref;
                n = s->pref.size() * sizeof(uint32_t);
                break;
        case 7:
                src = s->pdev.probes;
                n = s->probes.size() * sizeof(vrt_probe);
                break;
        }
        *bytes = (int64_t)n;
        if (!out)
                return VRT_OK;
        if (cap < (int64_t)n)
                return fail(VRT_E_INVALID, "vrt_scene_device_array: %lld bytes do not fit %lld", (long long)n,
                            (long long)cap);
        HIPCHK(hipSetDevice(s->device));
        if (n)
                HIPCHK(hipMemcpy(out, src, n, hipMemcpyDeviceToHost));
        return VRT_OK;
}

// ---- scene digest (vrt_digest.hip) -----------------------------------------
static uint64_t digest_words(const unsigned char *b, uint64_t W)
{
        uint64_t sum = 0;
        for (uint64_t i = 0; i < W; ++i) {
                const uint32_t w = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 |
                                   (uint32_t)b[4 * i + 3] << 24;
                uint64_t z = ((i + 1) * 0x9E3779B97F4A7C15ull) ^ (uint64_t)w;
                z ^= z >> 30;
                z *= 0xBF58476D1CE4E5B9ull;
                z ^= z >> 27;
                z *= 0x94D049BB133111EBull;
                z ^= z >> 31;
                sum += z;
        }
        return sum;
}

extern "C" int vrt_digest_host(const void *bytes, int64_t nbytes, uint64_t *out)
{
        if (!out || nbytes < 0 || (nbytes > 0 && !bytes))
                return fail(VRT_E_INVALID, "vrt_digest_host: null argument or negative size");
        if (nbytes % 4)
                return fail(VRT_E_INVALID, "vrt_digest_host: %lld bytes are no whole number of 32-bit words",
                            (long long)nbytes);
        *out = digest_words(static_cast<const unsigned char *>(bytes), (uint64_t)nbytes / 4);
        return VRT_OK;
}

extern "C" int vrt_device_selftest_digest(int device, const void *bytes, int64_t nbytes, int misalign, uint64_t *out)
{
        if (device < 0)
                return vrt_digest_host(bytes, nbytes, out);
        if (!out || nbytes < 0 || (nbytes > 0 && !bytes))
                return fail(VRT_E_INVALID, "vrt_device_selftest_digest: null argument or negative size");
        if (nbytes % 4)
                return fail(VRT_E_INVALID, "vrt_device_selftest_digest: %lld bytes are no whole number of 32-bit words",
                            (long long)nbytes);
        if (misalign != 0 && misalign != 4 && misalign != 8 && misalign != 12)
                return fail(VRT_E_INVALID, "vrt_device_selftest_digest: misalign %d (0, 4, 8 or 12)", misalign);
        if (int rc = check_device(device))
                return rc;
        HIPCHK(hipSetDevice(device));
        DevMem buf, d_out;
        HIPCHK(buf.alloc((size_t)nbytes + 32));
        HIPCHK(d_out.alloc(sizeof(uint64_t)));
        if (nbytes)
                HIPCHK(hipMemcpy(buf.as<char>() + misalign, bytes, (size_t)nbytes, hipMemcpyHostToDevice));
        DigestItems it{};
        it.n = 1;
        it.p[0] = buf.as<char>() + misalign;
        it.bytes[0] = nbytes;
        HIPCHK(launch_digest(it, d_out.as<uint64_t>(), nullptr));
        HIPCHK(hipMemcpy(out, d_out, sizeof(uint64_t), hipMemcpyDeviceToHost));
        return VRT_OK;
}

extern "C" int vrt_scene_digest(vrt_scene *s, uint64_t out[VRT_DIGEST_ITEMS])
{
        if (s && need_device(s))
                return VRT_E_NODEVICE;
        if (!s || !out)
                return fail(VRT_E_INVALID, "null argument");
        static_assert(VRT_DIGEST_ITEMS == kDigestItems, "digest items");
        std::lock_guard<std::mutex> lk(s->mu);
        const size_t nr = s->ref_tri.size(), nn = s->nodes.size();
        const size_t nbox = s->rboxes ? nr * sizeof(RefBox) : 0;
        DigestItems it{};
        it.n = kDigestItems;
        const void *p[kDigestItems] = { s->dev.refs,
                                        static_cast<const char *>(s->dev.refs) - nbox,
                                        s->dev.xnodes,
                                        s->dev.tri_pos,
                                        s->dev.tri_attr,
                                        s->pdev.pnode,
                                        s->pdev.pref,
                                        s->pdev.probes,
                                        s->dev.nodes,
                                        s->dev.node_vox };
        const size_t bytes[kDigestItems] = { nr * (s->wide_leaves ? sizeof(RefRec64) : sizeof(RefRec48)),
                                             nbox,
                                             nn * sizeof(XNodeRec),
                                             (size_t)s->ntri * sizeof(TriPos),
                                             (size_t)s->ntri * sizeof(TriAttr),
                                             s->probes.empty() ? 0 : s->pnode.size() * sizeof(uint2),
                                             s->probes.empty() ? 0 : s->pref.size() * sizeof(uint32_t),
                                             s->probes.size() * sizeof(vrt_probe),
                                             nn * sizeof(NodeRec),
                                             nn * sizeof(uint32_t) };
        for (int k = 0; k < kDigestItems; ++k) {
                it.p[k] = bytes[k] ? p[k] : nullptr;
                it.bytes[k] = (int64_t)bytes[k];
        }
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(s->digest.need(kDigestItems * sizeof(uint64_t)));
        HIPCHK(launch_digest(it, s->digest.as<uint64_t>(), s->stream));
        HIPCHK(hipMemcpyAsync(out, s->digest, kDigestItems * sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
        return VRT_OK;
}
