// vrt_multi.cpp -- the multi-device frame of include/vrt.h (SURVEY §8(b),
// §8(e)): the reference's render_mt (VRT/camera.h:42-68) spreads one frame's
// 8x8 tiles over the CPU's threads; here the tiles are dealt over the GPUs of
// one node.  The scene is built once and replicated per device; each rank
// renders its share of the tile deal into a packed buffer on its own stream,
// one RCCL ncclGather brings the shares to rank 0 over xGMI (rank 0's share
// is rendered in place into the receive buffer), and rank 0 re-assembles the
// image with the same unpack kernel as the torch.distributed path of
// bench.py.  The collective is the frame's only exchange.
//
// VRT/x = /root/reference/VoxelRayTrace20190722/x
#include "../../include/vrt.h"
#include "vrt_error.h"
#include "vrt_internal.h"

#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace vrt;

struct vrt_multi {
        std::vector<int> devs;          // rank i -> HIP device
        std::vector<vrt_scene *> sc;    // rank i's replica of the scene
        std::vector<ncclComm_t> comm;   // ncclCommInitAll over devs (empty: virtual ranks)
        bool virt = false;              // VRT_TEST_VIRTUAL_RANKS: n ranks on one device, copies for the gather
        std::vector<Stream> st;         // rank i's render + collective stream
        std::vector<Event> ev;          // rank i: its part of a frame queued
        std::vector<DevMem> send;       // ranks >= 1: packed tile buffer (tpr * 192 floats)
        DevMem gath;                    // rank 0: n * tpr * 192 floats (its own share in place)
        size_t tpr_cap = 0;             // tiles per rank the buffers hold
        // config 5 (vrt_render_secondary_multi*): rank i's primary records, visibility
        // image and primary-hit counter (8 B) on its device, used on st[i]
        std::vector<DevMem> prim, vis, hits;
        size_t prim_cap = 0, vis_cap = 0;  // bytes every rank's prim / vis holds
        Staging img;                    // vrt_render_multi: image on rank 0's device, its pinned copy; on st[0]
        Event ev_in;                    // caller's stream -> rank 0's stream
        int light_mode = VRT_MULTI_LIGHT_REPLICATED;  // vrt_multi_set_light_mode
        std::vector<Event> ev_x;        // virtual ranks, sharded light pass: rank i has read the others' hit lists
        // vrt_multi_update: the distribution's events on st[0] (made by the first
        // device update) and the last update's {total, slowest rank, distribute, verify} ms
        Event up_d0, up_d1;
        double up_ms[4] = {};
        bool updated = false;
        std::mutex mu;
};

namespace {

#define HIPCHK(expr)                                                                              \
        do {                                                                                      \
                hipError_t e_ = (expr);                                                           \
                if (e_ != hipSuccess)                                                             \
                        return set_error(VRT_E_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)); \
        } while (0)

#define NCCLCHK(expr)                                                                             \
        do {                                                                                      \
                ncclResult_t r_ = (expr);                                                         \
                if (r_ != ncclSuccess)                                                            \
                        return set_error(VRT_E_DEVICE, "%s failed: %s", #expr, ncclGetErrorString(r_)); \
        } while (0)

// the caller's current device is restored on every return
struct DeviceGuard {
        int dev = -1;
        DeviceGuard() { (void)hipGetDevice(&dev); }
        ~DeviceGuard()
        {
                if (dev >= 0)
                        (void)hipSetDevice(dev);
        }
};

std::vector<int> mask_devices(uint32_t mask)
{
        std::vector<int> d;
        for (int i = 0; i < 32; ++i)
                if (mask & (1u << i))
                        d.push_back(i);
        return d;
}

void free_buffers(vrt_multi *m)
{
        for (size_t i = 0; i < m->send.size(); ++i)
                if (m->send[i]) {
                        (void)hipSetDevice(m->devs[i]);
                        m->send[i].reset();
                }
        if (m->gath) {
                (void)hipSetDevice(m->devs[0]);
                m->gath.reset();
        }
        m->tpr_cap = 0;
}

// config 5's per-rank scratch, each with its device current
void free_secondary(vrt_multi *m)
{
        for (size_t i = 0; i < m->prim.size(); ++i)
                if (m->prim[i] || m->vis[i] || m->hits[i]) {
                        (void)hipSetDevice(m->devs[i]);
                        m->prim[i].reset();
                        m->vis[i].reset();
                        m->hits[i].reset();
                }
        m->prim_cap = m->vis_cap = 0;
}

int sync_all(vrt_multi *m)
{
        for (size_t i = 0; i < m->st.size(); ++i)
                if (m->st[i]) {
                        HIPCHK(hipSetDevice(m->devs[i]));
                        HIPCHK(hipStreamSynchronize(m->st[i]));
                }
        return VRT_OK;
}

// The ranks' packed buffers into rank 0's receive buffer m->gath (rank-major,
// `count` floats each), after each rank's render on its stream; rank 0's
// stream then holds the complete buffer.
int gather(vrt_multi *m, size_t count)
{
        const int n = (int)m->devs.size();
        if (m->virt) {
                // VRT_TEST_VIRTUAL_RANKS: rank i's buffer into its slot on rank
                // i's stream (after its render, where the collective's send
                // runs), and -- as the collective waits for the root -- only
                // once rank 0's stream has reached this frame's gather (so the
                // previous frame's unpack has read the slot); rank 0's stream
                // then waits for every copy
                HIPCHK(hipSetDevice(m->devs[0]));
                HIPCHK(hipEventRecord(m->ev[0], m->st[0]));
                for (int i = 1; i < n; ++i)
                        HIPCHK(hipStreamWaitEvent(m->st[i], m->ev[0], 0));
                for (int i = 1; i < n; ++i) {
                        HIPCHK(hipMemcpyAsync(m->gath.as<float>() + (size_t)i * count, m->send[i], count * sizeof(float),
                                              hipMemcpyDeviceToDevice, m->st[i]));
                        HIPCHK(hipEventRecord(m->ev[i], m->st[i]));
                        HIPCHK(hipStreamWaitEvent(m->st[0], m->ev[i], 0));
                }
                return VRT_OK;
        }
        // one RCCL gather to rank 0 (in place for rank 0: sendbuff == recvbuff + 0)
        NCCLCHK(ncclGroupStart());
        for (int i = 0; i < n; ++i) {
                const ncclResult_t r = ncclGather(i == 0 ? m->gath.get() : m->send[i].get(), i == 0 ? m->gath.get() : nullptr, count,
                                                  ncclFloat32, 0, m->comm[i], m->st[i]);
                if (r != ncclSuccess) {
                        (void)ncclGroupEnd();
                        return set_error(VRT_E_DEVICE, "ncclGather (rank %d): %s", i, ncclGetErrorString(r));
                }
        }
        NCCLCHK(ncclGroupEnd());
        return VRT_OK;
}

// What every rank enqueues for one frame: dst[i] is rank i's packed tile
// buffer (tpr * 64 * comps floats, written on m->st[i]), or null when the film
// has no tile.  It enqueues nothing collective, and after a failure it has
// synchronised whatever it started.
using RankWork = std::function<int(const std::vector<float *> &dst)>;

// One frame of `comps` floats per pixel (3: RGB, 1: config 5's visibility)
// into d_image on rank 0's device (caller holds m->mu): the ranks' work, the
// gather, the unpack.
int frame_multi(vrt_multi *m, const vrt_film *film, int comps, float *d_image, hipStream_t caller,
                const RankWork &work)
{
        const int n = (int)m->devs.size();
        const int tpr = vrt_tiles_per_rank(film, n);
        const size_t count = (size_t)tpr * 64 * comps;  // floats per rank buffer (8x8 pixels x comps per tile)
        if (tpr > 0 && (size_t)tpr > m->tpr_cap) {
                if (int rc = sync_all(m))
                        return rc;
                free_buffers(m);
                const size_t cap = (size_t)tpr * 192;  // room for either kind of frame
                for (int i = 1; i < n; ++i) {
                        HIPCHK(hipSetDevice(m->devs[i]));
                        HIPCHK(m->send[i].alloc(cap * sizeof(float)));
                }
                HIPCHK(hipSetDevice(m->devs[0]));
                HIPCHK(m->gath.alloc((size_t)n * cap * sizeof(float)));
                m->tpr_cap = (size_t)tpr;
        }
        HIPCHK(hipSetDevice(m->devs[0]));
        if (caller) {  // rank 0's stream follows the caller's
                HIPCHK(hipEventRecord(m->ev_in, caller));
                HIPCHK(hipStreamWaitEvent(m->st[0], m->ev_in, 0));
        }
        // each rank's share, packed tile-major
        std::vector<float *> dst(n, nullptr);
        if (tpr > 0)
                for (int i = 0; i < n; ++i)
                        dst[i] = (i == 0 ? m->gath : m->send[i]).as<float>();
        if (int rc = work(dst))
                return rc;
        if (tpr > 0)
                if (int rc = gather(m, count))
                        return rc;
        HIPCHK(hipSetDevice(m->devs[0]));
        if (tpr > 0) {
                if (int rc = comps == 3 ? vrt_unpack_tiles_device(film, n, m->gath.as<float>(), d_image, m->st[0])
                                        : vrt_unpack_tiles_c_device(film, n, comps, m->gath.as<float>(), d_image,
                                                                    m->st[0]))
                        return rc;
        } else {
                HIPCHK(hipMemsetAsync(d_image, 0, (size_t)film->nx * film->ny * comps * sizeof(float), m->st[0]));
        }
        if (caller) {
                HIPCHK(hipEventRecord(m->ev[0], m->st[0]));
                HIPCHK(hipStreamWaitEvent(caller, m->ev[0], 0));
        }
        return VRT_OK;
}

// A frame call's two outputs (comps floats per pixel): the host array rgb
// (through m->img), or d_image ordered on `stream` (null: complete on return).
// done (host output only): called under m->mu once every rank's stream is idle.
int frame_out(vrt_multi *m, const vrt_film *film, int comps, float *rgb, float *d_image, void *stream,
              const RankWork &work, const std::function<int()> &done = nullptr)
{
        std::lock_guard<std::mutex> lk(m->mu);
        DeviceGuard g;
        if (!rgb) {
                if (int rc = frame_multi(m, film, comps, d_image, static_cast<hipStream_t>(stream), work))
                        return rc;
                if (!stream)  // no caller stream: the image is complete on return
                        return sync_all(m);
                return VRT_OK;
        }
        const size_t bytes = (size_t)film->nx * film->ny * comps * sizeof(float);
        HIPCHK(hipSetDevice(m->devs[0]));
        HIPCHK(m->img.grow(bytes, m->st[0]));
        // the unpack writes every pixel (zero outside the tile grid)
        if (int rc = frame_multi(m, film, comps, m->img.d.as<float>(), nullptr, work))
                return rc;
        HIPCHK(hipSetDevice(m->devs[0]));
        HIPCHK(hipMemcpyAsync(m->img.h, m->img.d, bytes, hipMemcpyDeviceToHost, m->st[0]));
        if (int rc = sync_all(m))
                return rc;
        par_memcpy(rgb, m->img.h, bytes);
        return done ? done() : VRT_OK;
}

bool film_bad(const vrt_film *film)
{
        return film->nx < 1 || film->ny < 1 || film->nx > 32768 || film->ny > 32768;
}

// the primary frame: vrt_render_tiles_device with rank i of n
RankWork primary_work(vrt_multi *m, const vrt_camera *cam, const vrt_film *film)
{
        return [=](const std::vector<float *> &dst) -> int {
                for (size_t i = 0; i < dst.size(); ++i)
                        if (dst[i])
                                if (int rc = vrt_render_tiles_device(m->sc[i], cam, film, (int)i, (int)dst.size(), 0, dst[i],
                                                                     m->st[i]))
                                        return rc;
                return VRT_OK;
        };
}

// Every rank's streams (the handle's and the scenes') are idle; the error of
// the failed step stays the last error.
int fail_synced(vrt_multi *m, int rc)
{
        const std::string err = vrt_last_error();
        (void)sync_all(m);
        for (vrt_scene *s : m->sc)
                (void)scene_stream_sync(s);
        return set_error(rc, "%s", err.c_str());
}

// Config 5's scratch for this film on every rank (caller holds m->mu): the
// primary records, the visibility image and the hit counter.  Grown on
// demand, once every rank's stream is idle, as the tile buffers are.
int secondary_scratch(vrt_multi *m, const vrt_film *film)
{
        const size_t narea = (size_t)(8 * (film->nx / 8)) * (8 * (film->ny / 8));
        const size_t pb = narea * 8 * sizeof(float), vb = (size_t)film->nx * film->ny * sizeof(float);
        if (pb <= m->prim_cap && vb <= m->vis_cap && m->hits[0])
                return VRT_OK;
        if (int rc = sync_all(m))
                return rc;
        const size_t pcap = std::max(pb, m->prim_cap), vcap = std::max(vb, m->vis_cap);
        free_secondary(m);
        for (size_t i = 0; i < m->devs.size(); ++i) {
                HIPCHK(hipSetDevice(m->devs[i]));
                HIPCHK(m->prim[i].alloc(pcap));
                HIPCHK(m->vis[i].alloc(vcap));
                HIPCHK(m->hits[i].alloc(sizeof(uint64_t)));
        }
        m->prim_cap = pcap;
        m->vis_cap = vcap;
        return VRT_OK;
}

// the config-5 frame: vrt_render_secondary_tiles_device with rank i of n,
// into the handle's scratch and the rank's packed buffer
RankWork secondary_work(vrt_multi *m, const vrt_camera *cam, const vrt_film *film, int spp)
{
        return [=](const std::vector<float *> &dst) -> int {
                if (!dst[0])  // no tile: nothing to render
                        return VRT_OK;
                if (int rc = secondary_scratch(m, film))
                        return rc;
                for (size_t i = 0; i < dst.size(); ++i)
                        if (int rc = vrt_render_secondary_tiles_device(m->sc[i], cam, film, spp, (int)i, (int)dst.size(),
                                                                       m->prim[i].as<float>(), m->vis[i].as<float>(),
                                                                       dst[i], m->hits[i].as<uint64_t>(), m->st[i]))
                                return fail_synced(m, rc);
                return VRT_OK;
        };
}

int secondary_check(vrt_multi *m, const vrt_camera *cam, const vrt_film *film, int spp, const void *out)
{
        if (!m || !cam || !film || !out)
                return set_error(VRT_E_INVALID, "null argument");
        if (spp < 1 || spp > 64)
                return set_error(VRT_E_INVALID, "bad argument (spp must be 1..64)");
        if (film_bad(film))
                return set_error(VRT_E_INVALID, "bad film");
        return VRT_OK;
}

// Sharded light pass: every rank receives every other rank's keys and records
// behind its own (other ranks in rank order; order within the list is
// irrelevant), on the ranks' scene streams.  The source lists are complete:
// their counts were read after a stream sync.  A rank's stream goes on (to the
// sort, and later to the next march into the same lists) only when every other
// rank has read its list.
int exchange_lists(vrt_multi *m, const std::vector<LightList> &l)
{
        const int n = (int)l.size();
        if (m->virt) {
                HIPCHK(hipSetDevice(m->devs[0]));
                for (int d = 0; d < n; ++d) {
                        size_t off = l[d].n;
                        for (int r = 0; r < n; ++r) {
                                if (r == d || l[r].n == 0)
                                        continue;
                                HIPCHK(hipMemcpyAsync(l[d].keys + off, l[r].keys, (size_t)l[r].n * 8,
                                                      hipMemcpyDeviceToDevice, l[d].stream));
                                HIPCHK(hipMemcpyAsync(l[d].samp + 6 * off, l[r].samp, (size_t)l[r].n * 24,
                                                      hipMemcpyDeviceToDevice, l[d].stream));
                                off += l[r].n;
                        }
                        HIPCHK(hipEventRecord(m->ev_x[d], l[d].stream));
                }
                for (int r = 0; r < n; ++r)
                        for (int d = 0; d < n; ++d)
                                if (d != r)
                                        HIPCHK(hipStreamWaitEvent(l[r].stream, m->ev_x[d], 0));
                return VRT_OK;
        }
        // one broadcast of the keys and one of the records per root with hits
        // (zero-length ones skipped on all ranks alike), in one group; the
        // root's list stays in place
        NCCLCHK(ncclGroupStart());
        for (int r = 0; r < n; ++r) {
                if (l[r].n == 0)
                        continue;
                for (int i = 0; i < n; ++i) {
                        size_t off = 0;  // where root r's list lies on rank i
                        if (i != r) {
                                off = l[i].n;
                                for (int q = 0; q < r; ++q)
                                        if (q != i)
                                                off += l[q].n;
                        }
                        ncclResult_t e = ncclBroadcast(l[i].keys + off, l[i].keys + off, l[r].n, ncclUint64, r, m->comm[i],
                                                       l[i].stream);
                        if (e == ncclSuccess)
                                e = ncclBroadcast(l[i].samp + 6 * off, l[i].samp + 6 * off, (size_t)l[r].n * 6, ncclFloat32,
                                                  r, m->comm[i], l[i].stream);
                        if (e != ncclSuccess) {
                                (void)ncclGroupEnd();
                                return set_error(VRT_E_DEVICE, "ncclBroadcast (root %d, rank %d): %s", r, i,
                                                 ncclGetErrorString(e));
                        }
                }
        }
        NCCLCHK(ncclGroupEnd());
        return VRT_OK;
}

// The trace() frame's (or, with cam == nullptr or no tile, the light-map
// build's) per-rank work in its three steps, each on every rank before the
// next: the ranks' light passes run beside each other, not behind each
// other's host sync.  a: the call's arguments; rank, buffer and stream are
// filled in per rank.
int trace_work(vrt_multi *m, FrameArgs a, const std::vector<float *> &dst, int64_t *hits)
{
        const int n = (int)m->devs.size();
        const bool sharded = m->light_mode == VRT_MULTI_LIGHT_SHARDED && n > 1;
        const vrt_camera *cam = a.cam;
        std::vector<FrameJob *> job(n, nullptr);
        std::vector<LightList> l(n);
        auto bail = [&](int rc) {
                const std::string err = vrt_last_error();
                for (FrameJob *j : job)
                        frame_abort(j);
                (void)set_error(rc, "%s", err.c_str());
                return fail_synced(m, rc);
        };
        for (int i = 0; i < n; ++i) {
                a.cam = dst[i] ? cam : nullptr;
                a.rank = i;
                a.nranks = n;
                a.image_layout = 0;
                a.d_out = dst[i];
                a.stream = m->st[i];
                a.light_rank = sharded ? i : 0;
                a.light_nranks = sharded ? n : 1;
                if (int rc = frame_begin(m->sc[i], a, &job[i]))
                        return bail(rc);
        }
        for (int i = 0; i < n; ++i) {
                FrameJob *j = job[i];
                job[i] = nullptr;  // a failed step has released it
                if (int rc = frame_wait(j, &l[i]))
                        return bail(rc);
                job[i] = j;
        }
        uint64_t total = l[0].n;
        for (int i = 1; i < n; ++i) {
                if (sharded)
                        total += l[i].n;
                else if (l[i].n != l[0].n)
                        return bail(set_error(VRT_E_DEVICE, "replicas diverged: rank %d counts %u light hits, rank 0 %u", i,
                                              l[i].n, l[0].n));
        }
        if (total > l[0].cap)
                return bail(set_error(VRT_E_DEVICE, "light pass: %llu hits of %llu samples", (unsigned long long)total,
                                      (unsigned long long)l[0].cap));
        if (sharded)
                if (int rc = exchange_lists(m, l))
                        return bail(rc);
        for (int i = 0; i < n; ++i) {
                FrameJob *j = job[i];
                job[i] = nullptr;
                if (int rc = frame_finish(j, (unsigned int)total, sharded))
                        return bail(rc);
        }
        if (hits)
                *hits = (int64_t)total;
        return VRT_OK;
}

FrameArgs frame_args(const char *what, const vrt_camera *light_cam, const vrt_film *light_film,
                     const float *light_color, const vrt_camera *cam, const vrt_film *film, float min_voxel)
{
        FrameArgs a{};
        a.what = what;
        a.may_probe = true;
        a.light_cam = light_cam;
        a.light_film = light_film;
        a.light_color = light_color;
        a.light_nranks = 1;
        a.cam = cam;
        a.film = film;
        a.min_voxel = min_voxel;
        a.nranks = 1;
        return a;
}

int trace_frame_multi(vrt_multi *m, const char *what, const vrt_camera *light_cam, const vrt_film *light_film,
                      const float *light_color, const vrt_camera *cam, const vrt_film *film, float min_voxel,
                      float *rgb, float *d_image, void *stream, int64_t *hits)
{
        if (!m || !light_cam || !light_film || !cam || !film || !(rgb || d_image))
                return set_error(VRT_E_INVALID, "null argument");
        const FrameArgs a = frame_args(what, light_cam, light_film, light_color, cam, film, min_voxel);
        if (int rc = frame_check(m->sc[0], a))  // as every rank would, before anything is enqueued
                return rc;
        return frame_out(m, film, 3, rgb, d_image, stream,
                         [&](const std::vector<float *> &dst) { return trace_work(m, a, dst, hits); });
}

// the frame calls over a light list (vrt_lightmap_build_lights); cam ==
// nullptr: the light map alone
FrameArgs frame_args_lights(const char *what, const vrt_light *lights, int nlights, const float *probe_light_color,
                            const vrt_camera *cam, const vrt_film *film, float min_voxel)
{
        FrameArgs a = frame_args(what, nullptr, nullptr, probe_light_color, cam, film, min_voxel);
        a.lights = lights;
        a.nlights = nlights;
        return a;
}

int trace_frame_lights_multi(vrt_multi *m, const char *what, const vrt_light *lights, int nlights,
                             const float *probe_light_color, const vrt_camera *cam, const vrt_film *film,
                             float min_voxel, float *rgb, float *d_image, void *stream, int64_t *hits)
{
        if (!m || !lights || !cam || !film || !(rgb || d_image))
                return set_error(VRT_E_INVALID, "null argument");
        if (int rc = lights_ok(lights, nlights))
                return rc;
        const FrameArgs a = frame_args_lights(what, lights, nlights, probe_light_color, cam, film, min_voxel);
        if (int rc = frame_check(m->sc[0], a))  // as every rank would, before anything is enqueued
                return rc;
        return frame_out(m, film, 3, rgb, d_image, stream,
                         [&](const std::vector<float *> &dst) { return trace_work(m, a, dst, hits); });
}

int render_trace_multi(vrt_multi *m, const char *what, const vrt_camera *cam, const vrt_film *film, float min_voxel,
                       float *rgb, float *d_image, void *stream)
{
        if (!m || !cam || !film || !(rgb || d_image))
                return set_error(VRT_E_INVALID, "null argument");
        if (int rc = frame_check(m->sc[0], frame_args(what, nullptr, nullptr, nullptr, cam, film, min_voxel)))
                return rc;
        for (size_t i = 0; i < m->sc.size(); ++i)
                if (!scene_has_lightmap(m->sc[i]))
                        return set_error(VRT_E_INVALID, "no light map on rank %d: call vrt_lightmap_build_multi first",
                                         (int)i);
        return frame_out(m, film, 3, rgb, d_image, stream, [&](const std::vector<float *> &dst) -> int {
                for (size_t i = 0; i < dst.size(); ++i)
                        if (dst[i])
                                if (int rc = vrt_render_trace_probes_device(m->sc[i], cam, film, min_voxel, (int)i,
                                                                            (int)dst.size(), 0, dst[i], m->st[i]))
                                        return fail_synced(m, rc);
                return VRT_OK;
        });
}

// ---- vrt_multi_update ------------------------------------------------------
double now_ms()
{
        using namespace std::chrono;
        return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// f(rank) for every rank on a host thread of its own (rank 0 on the caller's),
// each with its status and its thread's vrt_last_error()
void for_ranks(int n, std::vector<int> &rcs, std::vector<std::string> &errs, const std::function<int(int)> &f)
{
        rcs.assign(n, VRT_OK);
        errs.assign(n, std::string());
        auto run = [&](int i) {
                rcs[i] = f(i);
                if (rcs[i])
                        errs[i] = vrt_last_error();
        };
        std::vector<std::thread> th;
        for (int i = 1; i < n; ++i)
                th.emplace_back(run, i);
        run(0);
        for (auto &t : th)
                t.join();
}

// The caller's device arrays (rank 0's device, complete once st[0] reaches this
// point) into the staging of every rank >= 1, on the ranks' handle streams;
// timed by up_d0 / up_d1 on st[0].  src / dst[i] / bytes: positions, normals,
// probes (bytes 0: not passed).
int distribute(vrt_multi *m, const void *const src[3], const std::vector<std::array<void *, 3>> &dst,
               const size_t bytes[3])
{
        const int n = (int)m->devs.size();
        HIPCHK(hipSetDevice(m->devs[0]));
        HIPCHK(hipEventRecord(m->up_d0, m->st[0]));
        if (m->virt) {
                // as gather() orders its copies: rank i's stream waits for rank
                // 0's, copies, and rank 0's stream waits for every copy
                HIPCHK(hipEventRecord(m->ev[0], m->st[0]));
                for (int i = 1; i < n; ++i)
                        HIPCHK(hipStreamWaitEvent(m->st[i], m->ev[0], 0));
                for (int i = 1; i < n; ++i) {
                        for (int k = 0; k < 3; ++k)
                                if (bytes[k])
                                        HIPCHK(hipMemcpyAsync(dst[i][k], src[k], bytes[k], hipMemcpyDeviceToDevice,
                                                              m->st[i]));
                        HIPCHK(hipEventRecord(m->ev[i], m->st[i]));
                        HIPCHK(hipStreamWaitEvent(m->st[0], m->ev[i], 0));
                }
        } else {
                // one broadcast of bytes per array from rank 0 (in place there)
                NCCLCHK(ncclGroupStart());
                for (int k = 0; k < 3; ++k) {
                        if (!bytes[k])
                                continue;
                        for (int i = 0; i < n; ++i) {
                                void *buf = i == 0 ? const_cast<void *>(src[k]) : dst[i][k];
                                const ncclResult_t e = ncclBroadcast(buf, buf, bytes[k], ncclUint8, 0, m->comm[i], m->st[i]);
                                if (e != ncclSuccess) {
                                        (void)ncclGroupEnd();
                                        return set_error(VRT_E_DEVICE, "ncclBroadcast (array %d, rank %d): %s", k, i,
                                                         ncclGetErrorString(e));
                                }
                        }
                }
                NCCLCHK(ncclGroupEnd());
                HIPCHK(hipSetDevice(m->devs[0]));
        }
        HIPCHK(hipEventRecord(m->up_d1, m->st[0]));
        return VRT_OK;
}

// VRT_MULTI_UPDATE_VERIFY: every rank's digest on its stream, then the ten
// words and the host-side constants of every rank against rank 0's
int verify_replicas(vrt_multi *m)
{
        static const char *const kItem[VRT_DIGEST_ITEMS] = { "leaf records", "per-record boxes", "xnodes", "TriPos",
                                                             "TriAttr",      "pnode",            "pref",   "probes",
                                                             "nodes",        "node_vox" };
        const int n = (int)m->devs.size();
        std::vector<std::array<uint64_t, VRT_DIGEST_ITEMS>> dig(n);
        std::vector<int> rcs;
        std::vector<std::string> errs;
        for_ranks(n, rcs, errs, [&](int i) { return vrt_scene_digest(m->sc[i], dig[i].data()); });
        for (int i = 0; i < n; ++i)
                if (rcs[i])
                        return set_error(rcs[i], "verify: rank %d (device %d): %s", i, m->devs[i], errs[i].c_str());
        vrt_scene_info_t i0{};
        int w0 = 0;
        float c0[3];
        if (int rc = vrt_scene_info(m->sc[0], &i0))
                return rc;
        scene_replica_key(m->sc[0], &w0, c0);
        for (int i = 1; i < n; ++i) {
                const char *what = nullptr;
                vrt_scene_info_t ii{};
                int wi = 0;
                float ci[3];
                if (int rc = vrt_scene_info(m->sc[i], &ii))
                        return rc;
                scene_replica_key(m->sc[i], &wi, ci);
                if (ii.nodes != i0.nodes || ii.internal != i0.internal || ii.leaves != i0.leaves ||
                    ii.nonempty_leaves != i0.nonempty_leaves || ii.tri_refs != i0.tri_refs)
                        what = "scene counts";
                else if (wi != w0)
                        what = "record format";
                else if (std::memcmp(ii.root_min, i0.root_min, sizeof i0.root_min) ||
                         std::memcmp(ii.root_max, i0.root_max, sizeof i0.root_max))
                        what = "root box";
                else if (std::memcmp(ci, c0, sizeof c0))
                        what = "chain spacing";
                for (int k = 0; !what && k < VRT_DIGEST_ITEMS; ++k)
                        if (dig[i][k] != dig[0][k])
                                what = kItem[k];
                if (what)
                        return set_error(VRT_E_DEVICE, "replicas diverged: rank %d (device %d), %s", i, m->devs[i], what);
        }
        return VRT_OK;
}

int multi_update(vrt_multi *m, const char *what, const float *pos, const float *nrm, const vrt_probe *probes,
                 int flags, bool on_device, hipStream_t caller)
{
        if (!m || !pos)
                return set_error(VRT_E_INVALID, "%s: null argument", what);
        if (flags & ~VRT_MULTI_UPDATE_VERIFY)
                return set_error(VRT_E_INVALID, "%s: unknown flags %#x", what, flags);
        std::lock_guard<std::mutex> lk(m->mu);
        DeviceGuard g;
        const int n = (int)m->devs.size();
        // the arguments once, as every rank would, before anything is enqueued
        if (int rc = update_multi_args_ok(m->sc[0], pos, probes != nullptr, what))
                return rc;
        if (probes && !on_device)
                if (int rc = update_probes_ok(probes, scene_nprobe(m->sc[0])))
                        return rc;
        const double t0 = now_ms();
        const int tf = test_flags();
        // what each rank reads, and the stream that orders it
        std::vector<const float *> rpos(n, pos), rnrm(n, nrm);
        std::vector<const vrt_probe *> rprobes(n, probes);
        std::vector<hipStream_t> rst(n, nullptr);
        bool distributed = false;
        std::vector<UpdatePlan> plans(n);
        std::vector<int> rcs;
        std::vector<std::string> errs;
        {
                // every rank scene is the update's from here to the commit's end
                std::vector<std::unique_lock<std::mutex>> held;
                for (vrt_scene *s : m->sc)
                        held.emplace_back(scene_mutex(s));
                if (on_device) {
                        // staging on the other ranks first: an allocation can refuse
                        std::vector<std::array<void *, 3>> dst(n);
                        size_t bytes[3] = {};
                        for (int i = 1; i < n; ++i) {
                                float *dp = nullptr, *dn = nullptr;
                                vrt_probe *dq = nullptr;
                                if (int rc = update_stage(m->sc[i], nrm != nullptr, probes != nullptr, &dp, &dn, &dq, bytes)) {
                                        const std::string err = vrt_last_error();
                                        return set_error(rc, "%s: rank %d (device %d): %s", what, i, m->devs[i],
                                                         err.c_str());
                                }
                                dst[i] = { dp, dn, dq };
                                rpos[i] = dp;
                                rnrm[i] = dn;
                                rprobes[i] = dq;
                        }
                        HIPCHK(hipSetDevice(m->devs[0]));
                        if (!m->up_d0) {
                                HIPCHK(m->up_d0.create());
                                HIPCHK(m->up_d1.create());
                        }
                        // rank 0's stream follows the caller's; every rank then reads
                        // its arrays in its handle stream's order
                        HIPCHK(hipEventRecord(m->ev_in, caller));
                        HIPCHK(hipStreamWaitEvent(m->st[0], m->ev_in, 0));
                        for (int i = 0; i < n; ++i)
                                rst[i] = m->st[i];
                        if (n > 1) {
                                const void *const src[3] = { pos, nrm, probes };
                                if (int rc = distribute(m, src, dst, bytes)) {
                                        held.clear();
                                        return fail_synced(m, rc);
                                }
                                distributed = true;
                        }
                }
                // 1. everything that can refuse, on every rank
                for_ranks(n, rcs, errs, [&](int i) {
                        const bool limit = (tf & VRT_TEST_UPDATE_TOO_LARGE) != 0 ||
                                           ((tf & VRT_TEST_MULTI_REFUSE_LAST) != 0 && i == n - 1);
                        return update_prepare(m->sc[i], rpos[i], rnrm[i], rprobes[i], on_device, rst[i], limit, &plans[i]);
                });
                for (int i = 0; i < n; ++i)
                        if (rcs[i]) {
                                // all ranks or none: every plan is abandoned, no rank has
                                // written an array that a frame reads
                                plans.clear();
                                held.clear();
                                (void)set_error(rcs[i], "%s: rank %d (device %d): %s", what, i, m->devs[i], errs[i].c_str());
                                return fail_synced(m, rcs[i]);
                        }
                // 2. the commit, which only a failed launch or copy can stop
                for_ranks(n, rcs, errs, [&](int i) { return update_commit(m->sc[i], &plans[i]); });
                for (int i = 0; i < n; ++i)
                        if (rcs[i]) {
                                held.clear();
                                (void)set_error(rcs[i], "%s: rank %d (device %d) half rebuilt, destroy the handle: %s", what,
                                                i, m->devs[i], errs[i].c_str());
                                return fail_synced(m, rcs[i]);
                        }
        }
        if (int rc = sync_all(m))  // the handle's streams: the distribution is over
                return rc;
        double ms[4] = {};
        for (vrt_scene *s : m->sc) {
                double r[4];
                if (int rc = vrt_scene_update_stats(s, r))
                        return rc;
                ms[1] = std::max(ms[1], r[0]);
        }
        if (distributed) {
                float d = 0.f;
                HIPCHK(hipSetDevice(m->devs[0]));
                HIPCHK(hipEventElapsedTime(&d, m->up_d0, m->up_d1));
                ms[2] = d;
        }
        if ((tf & VRT_TEST_MULTI_DIVERGE) != 0)
                if (int rc = scene_test_flip_attr(m->sc[n - 1]))
                        return rc;
        if (flags & VRT_MULTI_UPDATE_VERIFY) {
                const double v0 = now_ms();
                if (int rc = verify_replicas(m))
                        return rc;
                ms[3] = now_ms() - v0;
        }
        ms[0] = now_ms() - t0;
        std::memcpy(m->up_ms, ms, sizeof ms);
        m->updated = true;
        return VRT_OK;
}

}  // namespace

extern "C" void vrt_multi_destroy(vrt_multi *m)
{
        if (!m)
                return;
        DeviceGuard g;
        (void)sync_all(m);
        for (ncclComm_t c : m->comm)
                if (c)
                        (void)ncclCommDestroy(c);
        // each rank's resources go with its device current
        free_buffers(m);
        free_secondary(m);
        for (size_t i = 0; i < m->st.size(); ++i) {
                (void)hipSetDevice(m->devs[i]);
                m->ev[i].reset();
                if (i < m->ev_x.size())
                        m->ev_x[i].reset();
                m->st[i].reset();
        }
        for (vrt_scene *s : m->sc)
                vrt_scene_destroy(s);
        if (m->img.d || m->ev_in)  // rank 0's image pair and event
                (void)hipSetDevice(m->devs[0]);
        delete m;
}

// probes == nullptr: vrt_scene_create_multi (no probe flag); else a probe
// scene with vrt_scene_create_probes' flags
static int create_multi(const vrt_scene_desc *desc, const vrt_probe *probes, int32_t nprobe, int max_depth,
                        uint32_t device_mask, int flags, vrt_multi **out)
{
        if (!out)
                return set_error(VRT_E_INVALID, "null out");
        *out = nullptr;
        std::vector<int> devs = mask_devices(device_mask);
        if (devs.empty())
                return set_error(VRT_E_INVALID, "empty device mask");
        const int tf = test_flags();
        const bool virt = (tf & VRT_TEST_VIRTUAL_RANKS) != 0;
        if (virt) {
                const int nv = (tf >> 8) & 0xff;
                if (devs.size() != 1 || nv < 2 || nv > 16)
                        return set_error(VRT_E_INVALID, "virtual ranks need a one-device mask and 2..16 ranks (got %d)", nv);
                devs.assign(nv, devs[0]);
        }
        int nvis = 0;
        if (hipGetDeviceCount(&nvis) != hipSuccess || devs.back() >= nvis)
                return set_error(VRT_E_NODEVICE, "device mask %#x names device %d, %d visible", device_mask,
                                 devs.back(), nvis);
        DeviceGuard g;
        std::unique_ptr<vrt_multi, void (*)(vrt_multi *)> m(new (std::nothrow) vrt_multi, vrt_multi_destroy);
        if (!m)
                return set_error(VRT_E_NOMEM, "vrt_multi alloc");
        const int n = (int)devs.size();
        m->devs = devs;
        m->sc.assign(n, nullptr);
        m->st.resize(n);
        m->ev.resize(n);
        m->send.resize(n);
        m->ev_x.resize(n);
        m->prim.resize(n);
        m->vis.resize(n);
        m->hits.resize(n);
        // without probes VRT_BUILD_DEVICE_PROBES is refused too
        if (!probes && (flags & ~VRT_BUILD_DEVICE))
                return set_error(VRT_E_INVALID, "vrt_scene_create_multi: unknown flags %#x", flags);
        if (probes && flags != 0 && flags != (VRT_BUILD_DEVICE | VRT_BUILD_DEVICE_PROBES))
                return set_error(VRT_E_INVALID, "vrt_scene_create_multi_probes: flags %#x (0, or VRT_BUILD_DEVICE | "
                                                "VRT_BUILD_DEVICE_PROBES)", flags);
        // build once (host, or rank 0's device with VRT_BUILD_DEVICE) ...
        if (int rc = probes ? vrt_scene_create_probes(desc, probes, nprobe, max_depth, devs[0], flags, &m->sc[0])
                            : vrt_scene_create_ex(desc, max_depth, devs[0], flags, &m->sc[0]))
                return rc;
        // ... and upload the same build to every other device, in parallel
        std::vector<int> rcs(n, VRT_OK);
        std::vector<std::string> errs(n);
        {
                std::vector<std::thread> th;
                for (int i = 1; i < n; ++i)
                        th.emplace_back([&, i] {
                                rcs[i] = scene_replicate(m->sc[0], desc, devs[i], &m->sc[i]);
                                if (rcs[i])
                                        errs[i] = vrt_last_error();
                        });
                for (auto &t : th)
                        t.join();
        }
        for (int i = 1; i < n; ++i)
                if (rcs[i])
                        return set_error(rcs[i], "replica on device %d: %s", devs[i], errs[i].c_str());
        for (int i = 0; i < n; ++i) {
                scene_mark_owned(m->sc[i]);  // the ranks stay replicas: no vrt_scene_update
                HIPCHK(hipSetDevice(devs[i]));
                HIPCHK(m->st[i].create());
                HIPCHK(m->ev[i].create(hipEventDisableTiming));
                HIPCHK(m->ev_x[i].create(hipEventDisableTiming));
        }
        HIPCHK(hipSetDevice(devs[0]));
        HIPCHK(m->ev_in.create(hipEventDisableTiming));
        m->virt = virt;
        if (!virt) {
                m->comm.assign(n, nullptr);
                NCCLCHK(ncclCommInitAll(m->comm.data(), n, m->devs.data()));
        }
        *out = m.release();
        return VRT_OK;
}

extern "C" int vrt_scene_create_multi(const vrt_scene_desc *desc, int max_depth, uint32_t device_mask, int flags,
                                      vrt_multi **out)
{
        return create_multi(desc, nullptr, 0, max_depth, device_mask, flags, out);
}

extern "C" int vrt_scene_create_multi_probes(const vrt_scene_desc *desc, const vrt_probe *probes, int32_t nprobe,
                                             int max_depth, uint32_t device_mask, int flags, vrt_multi **out)
{
        if (nprobe == 0 || !probes)
                return create_multi(desc, nullptr, 0, max_depth, device_mask, flags, out);
        return create_multi(desc, probes, nprobe, max_depth, device_mask, flags, out);
}

extern "C" int vrt_multi_devices(const vrt_multi *m, int *n, int32_t *devices)
{
        if (!m || !n)
                return set_error(VRT_E_INVALID, "null argument");
        *n = (int)m->devs.size();
        if (devices)
                for (size_t i = 0; i < m->devs.size(); ++i)
                        devices[i] = m->devs[i];
        return VRT_OK;
}

extern "C" int vrt_multi_scene(vrt_multi *m, int rank, vrt_scene **out)
{
        if (!m || !out || rank < 0 || rank >= (int)m->sc.size())
                return set_error(VRT_E_INVALID, "bad argument");
        *out = m->sc[rank];
        return VRT_OK;
}

extern "C" int vrt_render_multi_device(vrt_multi *m, const vrt_camera *cam, const vrt_film *film, float *d_image,
                                       void *stream)
{
        if (!m || !cam || !film || !d_image)
                return set_error(VRT_E_INVALID, "null argument");
        if (film_bad(film))
                return set_error(VRT_E_INVALID, "bad film");
        return frame_out(m, film, 3, nullptr, d_image, stream, primary_work(m, cam, film));
}

extern "C" int vrt_render_multi(vrt_multi *m, const vrt_camera *cam, const vrt_film *film, float *rgb)
{
        if (!m || !cam || !film || !rgb)
                return set_error(VRT_E_INVALID, "null argument");
        if (film_bad(film))
                return set_error(VRT_E_INVALID, "bad film");
        return frame_out(m, film, 3, rgb, nullptr, nullptr, primary_work(m, cam, film));
}

extern "C" int vrt_render_secondary_multi_device(vrt_multi *m, const vrt_camera *cam, const vrt_film *film, int spp,
                                                 float *d_vis, void *stream)
{
        if (int rc = secondary_check(m, cam, film, spp, d_vis))
                return rc;
        return frame_out(m, film, 1, nullptr, d_vis, stream, secondary_work(m, cam, film, spp));
}

extern "C" int vrt_render_secondary_multi(vrt_multi *m, const vrt_camera *cam, const vrt_film *film, int spp,
                                          float *vis, int64_t *rays)
{
        if (int rc = secondary_check(m, cam, film, spp, vis))
                return rc;
        return frame_out(m, film, 1, vis, nullptr, nullptr, secondary_work(m, cam, film, spp), [&]() -> int {
                if (!rays)
                        return VRT_OK;
                // every rank's stream is idle: its counter is this frame's
                const int64_t narea = (int64_t)(8 * (film->nx / 8)) * (8 * (film->ny / 8));
                int64_t hits = 0;
                if (narea)
                        for (size_t i = 0; i < m->devs.size(); ++i) {
                                uint64_t h = 0;
                                HIPCHK(hipSetDevice(m->devs[i]));
                                HIPCHK(hipMemcpy(&h, m->hits[i], sizeof h, hipMemcpyDeviceToHost));
                                hits += (int64_t)h;
                        }
                *rays = narea + hits * spp;
                return VRT_OK;
        });
}

extern "C" int vrt_multi_set_light_mode(vrt_multi *m, int mode)
{
        if (!m)
                return set_error(VRT_E_INVALID, "null argument");
        if (mode != VRT_MULTI_LIGHT_REPLICATED && mode != VRT_MULTI_LIGHT_SHARDED)
                return set_error(VRT_E_INVALID, "unknown light mode %d", mode);
        std::lock_guard<std::mutex> lk(m->mu);
        m->light_mode = mode;
        return VRT_OK;
}

extern "C" int vrt_multi_set_probe_sgs(vrt_multi *m, const vrt_sg *sgs)
{
        if (!m || !sgs)
                return set_error(VRT_E_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(m->mu);
        DeviceGuard g;
        for (vrt_scene *s : m->sc)
                if (int rc = vrt_scene_set_probe_sgs(s, sgs))
                        return rc;
        return VRT_OK;
}

extern "C" int vrt_lightmap_build_multi(vrt_multi *m, const vrt_camera *light_cam, const vrt_film *light_film,
                                        int64_t *hits)
{
        if (!m || !light_cam || !light_film)
                return set_error(VRT_E_INVALID, "null argument");
        if (film_bad(light_film))
                return set_error(VRT_E_INVALID, "bad film");
        std::lock_guard<std::mutex> lk(m->mu);
        DeviceGuard g;
        const FrameArgs a = frame_args("vrt_lightmap_build_multi", light_cam, light_film, nullptr, nullptr, nullptr, 0.f);
        if (int rc = trace_work(m, a, std::vector<float *>(m->sc.size(), nullptr), hits))
                return rc;
        for (vrt_scene *s : m->sc)  // every rank's map is built on return
                if (int rc = scene_stream_sync(s))
                        return rc;
        return VRT_OK;
}

extern "C" int vrt_lightmap_build_lights_multi(vrt_multi *m, const vrt_light *lights, int nlights, int64_t *hits)
{
        if (!m || !lights)
                return set_error(VRT_E_INVALID, "null argument");
        if (int rc = lights_ok(lights, nlights))
                return rc;
        std::lock_guard<std::mutex> lk(m->mu);
        DeviceGuard g;
        const FrameArgs a = frame_args_lights("vrt_lightmap_build_lights_multi", lights, nlights, nullptr, nullptr,
                                              nullptr, 0.f);
        if (int rc = trace_work(m, a, std::vector<float *>(m->sc.size(), nullptr), hits))
                return rc;
        for (vrt_scene *s : m->sc)  // every rank's map is built on return
                if (int rc = scene_stream_sync(s))
                        return rc;
        return VRT_OK;
}

extern "C" int vrt_trace_frame_lights_multi(vrt_multi *m, const vrt_light *lights, int nlights,
                                            const float *probe_light_color, const vrt_camera *cam,
                                            const vrt_film *film, float min_voxel, float *rgb, int64_t *hits)
{
        return trace_frame_lights_multi(m, "vrt_trace_frame_lights_multi", lights, nlights, probe_light_color, cam, film,
                                        min_voxel, rgb, nullptr, nullptr, hits);
}

extern "C" int vrt_trace_frame_lights_multi_device(vrt_multi *m, const vrt_light *lights, int nlights,
                                                   const float *probe_light_color, const vrt_camera *cam,
                                                   const vrt_film *film, float min_voxel, float *d_image,
                                                   void *stream, int64_t *hits)
{
        return trace_frame_lights_multi(m, "vrt_trace_frame_lights_multi_device", lights, nlights, probe_light_color,
                                        cam, film, min_voxel, nullptr, d_image, stream, hits);
}

extern "C" int vrt_render_trace_multi(vrt_multi *m, const vrt_camera *cam, const vrt_film *film, float min_voxel,
                                      float *rgb)
{
        return render_trace_multi(m, "vrt_render_trace_multi", cam, film, min_voxel, rgb, nullptr, nullptr);
}

extern "C" int vrt_render_trace_multi_device(vrt_multi *m, const vrt_camera *cam, const vrt_film *film,
                                             float min_voxel, float *d_image, void *stream)
{
        return render_trace_multi(m, "vrt_render_trace_multi_device", cam, film, min_voxel, nullptr, d_image, stream);
}

extern "C" int vrt_trace_frame_multi(vrt_multi *m, const vrt_camera *light_cam, const vrt_film *light_film,
                                     const float *light_color, const vrt_camera *cam, const vrt_film *film,
                                     float min_voxel, float *rgb, int64_t *hits)
{
        return trace_frame_multi(m, "vrt_trace_frame_multi", light_cam, light_film, light_color, cam, film, min_voxel, rgb,
                                 nullptr, nullptr, hits);
}

extern "C" int vrt_trace_frame_multi_device(vrt_multi *m, const vrt_camera *light_cam, const vrt_film *light_film,
                                            const float *light_color, const vrt_camera *cam, const vrt_film *film,
                                            float min_voxel, float *d_image, void *stream, int64_t *hits)
{
        return trace_frame_multi(m, "vrt_trace_frame_multi_device", light_cam, light_film, light_color, cam, film,
                                 min_voxel, nullptr, d_image, stream, hits);
}

extern "C" int vrt_multi_tile_map(const vrt_film *film, uint32_t device_mask, int32_t *device_of_tile,
                                  int32_t *slot_of_tile)
{
        const std::vector<int> devs = mask_devices(device_mask);
        if (devs.empty() || !device_of_tile || !slot_of_tile)
                return set_error(VRT_E_INVALID, "bad argument");
        if (int rc = vrt_tile_deal_map(film, (int)devs.size(), device_of_tile, slot_of_tile))
                return rc;
        const int64_t nt = (int64_t)(film->nx / 8) * (film->ny / 8);
        for (int64_t t = 0; t < nt; ++t)
                device_of_tile[t] = devs[device_of_tile[t]];
        return VRT_OK;
}

extern "C" int vrt_multi_update(vrt_multi *m, const float *pos, const float *nrm, const vrt_probe *probes, int flags)
{
        return multi_update(m, "vrt_multi_update", pos, nrm, probes, flags, false, nullptr);
}

extern "C" int vrt_multi_update_device(vrt_multi *m, const float *d_pos, const float *d_nrm, const vrt_probe *d_probes,
                                       int flags, void *stream)
{
        return multi_update(m, "vrt_multi_update_device", d_pos, d_nrm, d_probes, flags, true,
                            static_cast<hipStream_t>(stream));
}

extern "C" int vrt_multi_update_stats(const vrt_multi *m, double ms[4])
{
        if (!m || !ms)
                return set_error(VRT_E_INVALID, "null argument");
        if (!m->updated)
                return set_error(VRT_E_INVALID, "the handle has not been updated");
        for (int k = 0; k < 4; ++k)
                ms[k] = m->up_ms[k];
        return VRT_OK;
}
