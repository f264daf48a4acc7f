// vrt_build.hip -- octree build on the GPU.
//
// Same octree as the host build (vrt_host.cpp: build_tree) and as the
// reference's recursive insert()/split() (VRT/voxel_octree.cc:27-75): a node
// at depth < max_depth is split iff some triangle overlaps it and all its
// ancestors (Triangle::is_overlap = triBoxOverlap on the node's exact float
// box, VRT/voxel_octree.cc:486-492); a max-depth leaf lists exactly those
// triangles, in input order.  Level-synchronous on the device:
//   frontier P_l = (triangle, node code, node box) pairs that overlap;
//   k_expand tests the 8 children of every pair (SAT) and appends the
//   overlapping ones to P_{l+1} (wave-aggregated atomics; order is
//   irrelevant because everything below is sorted);
//   internal nodes of level l = sorted unique codes of P_l (hipCUB);
//   leaf lists = sorted (code << 32 | tri) of P_max_depth.
// Then the BFS child-block layout is written top-down one level per launch
// (children boxes from the parent's stored box with split()'s float ops),
// and the content masks bottom-up.  Node boxes, codes, leaf lists and masks
// are identical to the host build (tests/test_gpu.py).
//
// Light probes (vrt_scene_create_probes with VRT_BUILD_DEVICE_PROBES) are a
// second frontier beside the triangles': (probe, node code, node box) pairs
// expanded with LightProbe::is_overlap (probe_overlap).  A level's internal
// nodes are the sorted unique codes of both frontiers together; the probes'
// leaf lists, sorted (code << 32 | probe), stay apart from the triangles' in
// the side arrays pnode / pref, as in the host build
// (tests/test_probe_build_gpu.py).  A scene without probes takes none of the
// probe launches.
#include <hipcub/hipcub.hpp>

#include "vrt_internal.h"

namespace vrt {

namespace {

struct alignas(16) Pair {
        float mn[3], mx[3];
        uint32_t tri, code;
};
static_assert(sizeof(Pair) == 32, "Pair must be 32 B");

// split() child box (VRT/voxel_octree.cc:30-35)
__device__ __forceinline__ void child_box_dev(const float *pmn, const float *pmx, int i, float *cmn, float *cmx)
{
        const int m[3] = { (i & 4) ? 1 : 0, (i & 2) ? 1 : 0, (i & 1) ? 1 : 0 };
#pragma unroll
        for (int k = 0; k < 3; ++k) {
                const float half = (pmx[k] - pmn[k]) / 2.0f;
                cmn[k] = pmn[k] + (float)m[k] * half;
                cmx[k] = cmn[k] + half;
        }
}

// Triangle::is_overlap (VRT/voxel_octree.cc:486-492)
__device__ __forceinline__ bool overlaps_dev(const float *tri9, const float *mn, const float *mx)
{
        float c[3], h[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
                c[k] = (mn[k] + mx[k]) * .5f;
                h[k] = (mx[k] - mn[k]) / 2.f;
        }
        return tri_box_overlap(c, h, tri9) == 1;
}

// Exclusive prefix of `cnt` over the wave plus one atomicAdd per wave.
__device__ __forceinline__ uint32_t wave_append(uint32_t cnt, unsigned int *counter)
{
        const int lane = threadIdx.x & 63;
        uint32_t incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
                const uint32_t v = __shfl_up(incl, o, 64);
                if (lane >= o)
                        incl += v;
        }
        uint32_t base = 0;
        if (lane == 63 && incl)
                base = atomicAdd(counter, incl);
        base = __shfl(base, 63, 64);
        return base + incl - cnt;
}

__global__ __launch_bounds__(256) void k_seed(int n, const float *__restrict__ pos, Pair root,
                                              Pair *__restrict__ out, unsigned int *counter)
{
        const int i = blockIdx.x * blockDim.x + threadIdx.x;
        float tri[9];
        bool hit = false;
        if (i < n) {
#pragma unroll
                for (int k = 0; k < 9; ++k)
                        tri[k] = pos[9 * (int64_t)i + k];
                hit = overlaps_dev(tri, root.mn, root.mx);
        }
        const uint32_t at = wave_append(hit ? 1u : 0u, counter);
        if (hit) {
                Pair p = root;
                p.tri = (uint32_t)i;
                p.code = 0;
                out[at] = p;
        }
}

__global__ __launch_bounds__(256) void k_expand(int64_t n, const Pair *__restrict__ in,
                                                const float *__restrict__ pos, uint32_t *__restrict__ codes,
                                                Pair *__restrict__ out, unsigned int *counter)
{
        const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        uint32_t mask = 0;
        Pair p;
        float cmn[8][3], cmx[8][3];
        if (i < n) {
                p = in[i];
                codes[i] = p.code;
                float tri[9];
                const float *t = pos + 9 * (int64_t)p.tri;
#pragma unroll
                for (int k = 0; k < 9; ++k)
                        tri[k] = t[k];
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                        child_box_dev(p.mn, p.mx, c, cmn[c], cmx[c]);
                        if (overlaps_dev(tri, cmn[c], cmx[c]))
                                mask |= 1u << c;
                }
        }
        uint32_t at = wave_append((uint32_t)__popc(mask), counter);
        if (mask) {
#pragma unroll
                for (int c = 0; c < 8; ++c)
                        if (mask & (1u << c)) {
                                Pair q;
#pragma unroll
                                for (int k = 0; k < 3; ++k) {
                                        q.mn[k] = cmn[c][k];
                                        q.mx[k] = cmx[c][k];
                                }
                                q.tri = p.tri;
                                q.code = (p.code << 3) | (uint32_t)c;
                                out[at++] = q;
                        }
        }
}

// The probe frontier: Pair::tri is the probe index.  A probe that misses the
// root (r == 0 among them) drops out here.
__global__ __launch_bounds__(256) void k_seed_probes(int n, const float4 *__restrict__ probes, Pair root,
                                                     Pair *__restrict__ out, unsigned int *counter)
{
        const int i = blockIdx.x * blockDim.x + threadIdx.x;
        bool hit = false;
        if (i < n) {
                const float4 pb = probes[i];
                hit = probe_overlap(mk3(pb.x, pb.y, pb.z), pb.w, root.mn, root.mx);
        }
        const uint32_t at = wave_append(hit ? 1u : 0u, counter);
        if (hit) {
                Pair p = root;
                p.tri = (uint32_t)i;
                p.code = 0;
                out[at] = p;
        }
}

// k_expand for the probe frontier: LightProbe::is_overlap on the 8 split()
// children.  `codes` is this frontier's part of the level's code array.
__global__ __launch_bounds__(256) void k_expand_probes(int64_t n, const Pair *__restrict__ in,
                                                       const float4 *__restrict__ probes,
                                                       uint32_t *__restrict__ codes, Pair *__restrict__ out,
                                                       unsigned int *counter)
{
        const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        uint32_t mask = 0;
        Pair p;
        float cmn[8][3], cmx[8][3];
        if (i < n) {
                p = in[i];
                codes[i] = p.code;
                const float4 pb = probes[p.tri];
                const f3 o = mk3(pb.x, pb.y, pb.z);
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                        child_box_dev(p.mn, p.mx, c, cmn[c], cmx[c]);
                        if (probe_overlap(o, pb.w, cmn[c], cmx[c]))
                                mask |= 1u << c;
                }
        }
        uint32_t at = wave_append((uint32_t)__popc(mask), counter);
        if (mask) {
#pragma unroll
                for (int c = 0; c < 8; ++c)
                        if (mask & (1u << c)) {
                                Pair q;
#pragma unroll
                                for (int k = 0; k < 3; ++k) {
                                        q.mn[k] = cmn[c][k];
                                        q.mx[k] = cmx[c][k];
                                }
                                q.tri = p.tri;
                                q.code = (p.code << 3) | (uint32_t)c;
                                out[at++] = q;
                        }
        }
}

__global__ __launch_bounds__(256) void k_leaf_keys(int64_t n, const Pair *__restrict__ in, uint64_t *__restrict__ keys)
{
        const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (i < n)
                keys[i] = ((uint64_t)in[i].code << 32) | in[i].tri;
}

__device__ __forceinline__ uint32_t vox_of_dev(uint32_t code, int depth)
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

template <class T>
__device__ __forceinline__ int64_t lower_bound_dev(const T *a, int64_t n, T key)
{
        int64_t lo = 0, hi = n;
        while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (a[mid] < key)
                        lo = mid + 1;
                else
                        hi = mid;
        }
        return lo;
}

struct FlatLevel {
        int level, max_depth;
        int64_t begin, count;     // node index range of this level
        const uint32_t *iall;     // internal codes, level by level, each sorted
        int64_t jg_base;          // global index of this level's first internal node
        int64_t n_int;            // internal nodes at this level
        uint32_t *inode_of;       // global internal index -> node index
        const uint64_t *refs;     // sorted (code << 32 | tri)
        int64_t nrefs;
        float root_mn[3], root_mx[3];
        NodeRec *nodes;
        uint32_t *node_vox;
};

__global__ __launch_bounds__(256) void k_flatten(FlatLevel f)
{
        const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (t >= f.count)
                return;
        const int64_t ni = f.begin + t;
        uint32_t code;
        float mn[3], mx[3];
        if (f.level == 1) {
                code = 0;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                        mn[k] = f.root_mn[k];
                        mx[k] = f.root_mx[k];
                }
        } else {
                const int64_t jp = (ni - 1) >> 3;
                const int c = (int)((ni - 1) & 7);
                const NodeRec &pn = f.nodes[f.inode_of[jp]];
                child_box_dev(pn.bmin, pn.bmax, c, mn, mx);
                code = (f.iall[jp] << 3) | (uint32_t)c;
        }
        NodeRec nr;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
                nr.bmin[k] = mn[k];
                nr.bmax[k] = mx[k];
        }
        nr.b = 0;
        if (f.level < f.max_depth) {
                const uint32_t *I = f.iall + f.jg_base;
                const int64_t r = lower_bound_dev<uint32_t>(I, f.n_int, code);
                if (r < f.n_int && I[r] == code) {
                        const int64_t jg = f.jg_base + r;
                        nr.a = (uint32_t)(1 + 8 * jg);
                        f.inode_of[jg] = (uint32_t)ni;
                } else {
                        nr.a = kLeafBit;  // empty leaf above max depth
                }
        } else {
                const uint64_t k0 = (uint64_t)code << 32;
                const int64_t lo = lower_bound_dev<uint64_t>(f.refs, f.nrefs, k0);
                const int64_t hi = lower_bound_dev<uint64_t>(f.refs, f.nrefs, k0 + (1ull << 32));
                nr.a = kLeafBit | (uint32_t)(hi - lo);
                nr.b = (uint32_t)lo;
        }
        f.nodes[ni] = nr;
        f.node_vox[ni] = vox_of_dev(code, f.level);
}

// content masks of one level, bottom-up (vrt_host.cpp: build_tree)
__global__ __launch_bounds__(256) void k_masks(int64_t begin, int64_t end, NodeRec *__restrict__ nodes,
                                               uint8_t *__restrict__ has)
{
        const int64_t ni = begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (ni >= end)
                return;
        NodeRec &nr = nodes[ni];
        if (nr.a & kLeafBit) {
                has[ni] = (nr.a & ~kLeafBit) ? 1 : 0;
                return;
        }
        uint32_t m = 0;
        for (int c = 0; c < 8; ++c)
                m |= (uint32_t)has[nr.a + c] << c;
        nr.b = m;
        has[ni] = m ? 1 : 0;
}

// pref = the probe indices of the sorted (code << 32 | probe) keys
__global__ __launch_bounds__(256) void k_pref(int64_t n, const uint64_t *__restrict__ keys,
                                              uint32_t *__restrict__ pref)
{
        const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (i < n)
                pref[i] = (uint32_t)(keys[i] & 0xFFFFFFFFu);
}

// k_flatten's leaf part for the probes: pnode = (first, count) of the
// max-depth leaves [begin, begin + count) in the sorted probe keys (pnode is
// zero elsewhere); *leaves counts those with a probe.
__global__ __launch_bounds__(256) void k_probe_leaves(int level, int64_t begin, int64_t count,
                                                      const uint32_t *__restrict__ iall,
                                                      const uint64_t *__restrict__ keys, int64_t nkeys,
                                                      uint2 *__restrict__ pnode, unsigned int *leaves)
{
        const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        uint32_t some = 0;
        if (t < count) {
                const int64_t ni = begin + t;
                const uint32_t code = level == 1 ? 0u : (iall[(ni - 1) >> 3] << 3) | (uint32_t)((ni - 1) & 7);
                const uint64_t k0 = (uint64_t)code << 32;
                const int64_t lo = lower_bound_dev<uint64_t>(keys, nkeys, k0);
                const int64_t hi = lower_bound_dev<uint64_t>(keys, nkeys, k0 + (1ull << 32));
                pnode[ni] = make_uint2((uint32_t)lo, (uint32_t)(hi - lo));
                some = hi > lo ? 1u : 0u;
        }
        (void)wave_append(some, leaves);
}

// k_masks for the probes: an internal node's pnode.x = the children with a
// probe somewhere below (vrt_host.cpp: build_tree)
__global__ __launch_bounds__(256) void k_probe_masks(int64_t begin, int64_t end, const NodeRec *__restrict__ nodes,
                                                     uint2 *__restrict__ pnode, uint8_t *__restrict__ has)
{
        const int64_t ni = begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (ni >= end)
                return;
        const uint32_t a = nodes[ni].a;
        if (a & kLeafBit) {
                has[ni] = pnode[ni].y ? 1 : 0;
                return;
        }
        uint32_t m = 0;
        for (int c = 0; c < 8; ++c)
                m |= (uint32_t)has[a + c] << c;
        pnode[ni] = make_uint2(m, 0u);
        has[ni] = m ? 1 : 0;
}

// a build array: never empty once allocated
struct Dev : DevMem {
        hipError_t alloc(size_t n) { return DevMem::alloc(n ? n : 16); }
};

#define BCHK(expr)                                                                           \
        do {                                                                                 \
                hipError_t e_ = (expr);                                                      \
                if (e_ != hipSuccess) {                                                      \
                        *err = std::string(#expr) + ": " + hipGetErrorString(e_);             \
                        return e_;                                                           \
                }                                                                            \
        } while (0)

// a size limit of the build: VRT_E_INVALID for the caller, not a device error
#define BLIMIT(cond, ...)                                                                    \
        do {                                                                                 \
                if (cond) {                                                                  \
                        char m_[160];                                                        \
                        std::snprintf(m_, sizeof m_, __VA_ARGS__);                           \
                        *err = m_;                                                           \
                        out->too_large = true;                                               \
                        return hipErrorInvalidValue;                                         \
                }                                                                            \
        } while (0)

unsigned grid_of(int64_t n)
{
        return (unsigned)((n + 255) / 256);
}

}  // namespace

hipError_t build_tree_device(int device, const float *pos, int ntri, const float root_mn[3],
                             const float root_mx[3], int D, const vrt_probe *probes, int nprobe, DeviceBuild *out,
                             std::string *err)
{
        static_assert(sizeof(vrt_probe) == sizeof(float4), "vrt_probe layout");
        BCHK(hipSetDevice(device));
        hipStream_t st = nullptr;
        Event e0, e1;
        BCHK(e0.create());
        BCHK(e1.create());
        Dev dpos, cnt, pa, pb, codes, codes_s, uniq, nuniq, temp, iall, keys, keys_s, inode, dnodes, dvox, dhas;
        Dev dprobes, qa, qb, pkeys, pkeys_s, dpref, dpnode, dphas;  // the probe frontier and its outputs
        BCHK(dpos.alloc((size_t)ntri * 36));
        BCHK(hipMemcpy(dpos, pos, (size_t)ntri * 36, hipMemcpyHostToDevice));
        if (nprobe > 0) {
                BCHK(dprobes.alloc((size_t)nprobe * sizeof(float4)));
                BCHK(hipMemcpy(dprobes, probes, (size_t)nprobe * sizeof(float4), hipMemcpyHostToDevice));
        }
        BCHK(hipEventRecord(e0, st));
        BCHK(cnt.alloc(16));
        Pair root;
        for (int k = 0; k < 3; ++k) {
                root.mn[k] = root_mn[k];
                root.mx[k] = root_mx[k];
        }
        root.tri = 0;
        root.code = 0;
        // level 1 frontier
        BCHK(pa.alloc((size_t)std::max(1, ntri) * sizeof(Pair)));
        BCHK(hipMemsetAsync(cnt, 0, 16, st));
        if (ntri > 0)
                hipLaunchKernelGGL(k_seed, dim3(grid_of(ntri)), dim3(256), 0, st, ntri, dpos.as<float>(), root,
                                   pa.as<Pair>(), cnt.as<unsigned int>());
        BCHK(hipGetLastError());
        unsigned int hn = 0;
        BCHK(hipMemcpy(&hn, cnt, 4, hipMemcpyDeviceToHost));
        int64_t n = hn;
        // the probes' counter is the second word of cnt
        unsigned int *const qcnt = cnt.as<unsigned int>() + 1;
        int64_t nq = 0;
        if (nprobe > 0) {
                BCHK(qa.alloc((size_t)nprobe * sizeof(Pair)));
                hipLaunchKernelGGL(k_seed_probes, dim3(grid_of(nprobe)), dim3(256), 0, st, nprobe,
                                   dprobes.as<float4>(), root, qa.as<Pair>(), qcnt);
                BCHK(hipGetLastError());
                BCHK(hipMemcpy(&hn, qcnt, 4, hipMemcpyDeviceToHost));
                nq = hn;
        }
        std::vector<uint32_t> h_iall;          // internal codes, level by level
        std::vector<int64_t> n_int(D + 1, 0);  // per level
        int64_t nrefs = 0, nprefs = 0;
        for (int l = 1; l <= D; ++l) {
                if (l == D) {
                        // probe leaf lists: sort (code << 32 | probe)
                        nprefs = nq;
                        if (nq > 0) {
                                BCHK(pkeys.alloc((size_t)nq * 8));
                                BCHK(pkeys_s.alloc((size_t)nq * 8));
                                hipLaunchKernelGGL(k_leaf_keys, dim3(grid_of(nq)), dim3(256), 0, st, nq, qa.as<Pair>(),
                                                   pkeys.as<uint64_t>());
                                BCHK(hipGetLastError());
                                size_t tb = 0;
                                const int bits = 32 + 3 * (D - 1);
                                BCHK(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, pkeys.as<uint64_t>(),
                                                                       pkeys_s.as<uint64_t>(), (int)nq, 0, bits, st));
                                BCHK(temp.alloc(tb));
                                BCHK(hipcub::DeviceRadixSort::SortKeys(temp, tb, pkeys.as<uint64_t>(),
                                                                       pkeys_s.as<uint64_t>(), (int)nq, 0, bits, st));
                        }
                        // leaf lists: sort (code << 32 | tri)
                        nrefs = n;
                        BCHK(keys.alloc((size_t)std::max<int64_t>(1, n) * 8));
                        BCHK(keys_s.alloc((size_t)std::max<int64_t>(1, n) * 8));
                        if (n > 0) {
                                hipLaunchKernelGGL(k_leaf_keys, dim3(grid_of(n)), dim3(256), 0, st, n, pa.as<Pair>(),
                                                   keys.as<uint64_t>());
                                BCHK(hipGetLastError());
                                size_t tb = 0;
                                const int bits = 32 + 3 * (D - 1);
                                BCHK(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, keys.as<uint64_t>(),
                                                                       keys_s.as<uint64_t>(), (int)n, 0, bits, st));
                                BCHK(temp.alloc(tb));
                                BCHK(hipcub::DeviceRadixSort::SortKeys(temp, tb, keys.as<uint64_t>(),
                                                                       keys_s.as<uint64_t>(), (int)n, 0, bits, st));
                        }
                        break;
                }
                // the append counters are 32-bit and hipCUB takes int counts
                BLIMIT(8 * n > 0x7FFFFFFF, "device octree build: %lld (triangle, node) pairs at level %d, 8 x that must stay below 2^31",
                       (long long)n, l);
                BLIMIT(8 * nq > 0x7FFFFFFF, "device octree build: %lld (probe, node) pairs at level %d, 8 x that must stay below 2^31",
                       (long long)nq, l);
                // expand: codes of this level (the triangles' pairs, then the
                // probes') + next frontiers
                const int64_t nc = n + nq;
                BCHK(codes.alloc((size_t)std::max<int64_t>(1, nc) * 4));
                BCHK(pb.alloc((size_t)std::max<int64_t>(1, 8 * n) * sizeof(Pair)));
                BCHK(hipMemsetAsync(cnt, 0, 16, st));
                if (n > 0)
                        hipLaunchKernelGGL(k_expand, dim3(grid_of(n)), dim3(256), 0, st, n, pa.as<Pair>(),
                                           dpos.as<float>(), codes.as<uint32_t>(), pb.as<Pair>(),
                                           cnt.as<unsigned int>());
                BCHK(hipGetLastError());
                if (nq > 0) {
                        BCHK(qb.alloc((size_t)(8 * nq) * sizeof(Pair)));
                        hipLaunchKernelGGL(k_expand_probes, dim3(grid_of(nq)), dim3(256), 0, st, nq, qa.as<Pair>(),
                                           dprobes.as<float4>(), codes.as<uint32_t>() + n, qb.as<Pair>(), qcnt);
                        BCHK(hipGetLastError());
                }
                // internal nodes of level l = sorted unique codes
                int64_t nu = 0;
                if (nc > 0) {
                        const int bits = std::max(1, 3 * (l - 1));
                        BCHK(codes_s.alloc((size_t)nc * 4));
                        BCHK(uniq.alloc((size_t)nc * 4));
                        BCHK(nuniq.alloc(8));
                        size_t tb = 0, tb2 = 0;
                        BCHK(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, codes.as<uint32_t>(), codes_s.as<uint32_t>(),
                                                               (int)nc, 0, bits, st));
                        BCHK(hipcub::DeviceSelect::Unique(nullptr, tb2, codes_s.as<uint32_t>(), uniq.as<uint32_t>(),
                                                          nuniq.as<int>(), (int)nc, st));
                        BCHK(temp.alloc(std::max(tb, tb2)));
                        BCHK(hipcub::DeviceRadixSort::SortKeys(temp, tb, codes.as<uint32_t>(), codes_s.as<uint32_t>(),
                                                               (int)nc, 0, bits, st));
                        BCHK(hipcub::DeviceSelect::Unique(temp, tb2, codes_s.as<uint32_t>(), uniq.as<uint32_t>(),
                                                          nuniq.as<int>(), (int)nc, st));
                        int hnu = 0;
                        BCHK(hipMemcpy(&hnu, nuniq, 4, hipMemcpyDeviceToHost));
                        nu = hnu;
                        const size_t o = h_iall.size();
                        h_iall.resize(o + (size_t)nu);
                        if (nu)
                                BCHK(hipMemcpy(h_iall.data() + o, uniq, (size_t)nu * 4, hipMemcpyDeviceToHost));
                }
                n_int[l] = nu;
                BCHK(hipMemcpy(&hn, cnt, 4, hipMemcpyDeviceToHost));
                n = hn;
                std::swap(pa, pb);
                if (nq > 0) {
                        BCHK(hipMemcpy(&hn, qcnt, 4, hipMemcpyDeviceToHost));
                        nq = hn;
                        std::swap(qa, qb);
                }
                if (nu == 0)
                        break;  // nothing below this level
        }
        // ---- flatten: level ranges as the host build (root, then 8 children
        // per internal node of the previous level, in code order)
        int64_t ninternal = (int64_t)h_iall.size();
        const int64_t nnodes = 1 + 8 * ninternal;
        BLIMIT(nnodes > 0x7FFFFFFF, "octree too large (%lld nodes)", (long long)nnodes);
        out->level_begin.clear();
        BCHK(iall.alloc(std::max<size_t>(1, h_iall.size()) * 4));
        if (!h_iall.empty())
                BCHK(hipMemcpy(iall, h_iall.data(), h_iall.size() * 4, hipMemcpyHostToDevice));
        BCHK(inode.alloc(std::max<int64_t>(1, ninternal) * 4));
        BCHK(dnodes.alloc((size_t)nnodes * sizeof(NodeRec)));
        BCHK(dvox.alloc((size_t)nnodes * 4));
        int64_t begin = 0, count = 1, jg_base = 0;
        for (int l = 1; l <= D && count > 0; ++l) {
                out->level_begin.push_back(begin);
                FlatLevel f;
                f.level = l;
                f.max_depth = D;
                f.begin = begin;
                f.count = count;
                f.iall = iall.as<uint32_t>();
                f.jg_base = jg_base;
                f.n_int = l < D ? n_int[l] : 0;
                f.inode_of = inode.as<uint32_t>();
                f.refs = keys_s.as<uint64_t>();
                f.nrefs = nrefs;
                for (int k = 0; k < 3; ++k) {
                        f.root_mn[k] = root_mn[k];
                        f.root_mx[k] = root_mx[k];
                }
                f.nodes = dnodes.as<NodeRec>();
                f.node_vox = dvox.as<uint32_t>();
                hipLaunchKernelGGL(k_flatten, dim3(grid_of(count)), dim3(256), 0, st, f);
                BCHK(hipGetLastError());
                begin += count;
                count = 8 * f.n_int;
                jg_base += f.n_int;
        }
        out->level_begin.push_back(nnodes);
        // content masks bottom-up
        BCHK(dhas.alloc((size_t)nnodes));
        for (int l = (int)out->level_begin.size() - 1; l >= 1; --l) {
                const int64_t b0 = out->level_begin[l - 1], b1 = out->level_begin[l];
                hipLaunchKernelGGL(k_masks, dim3(grid_of(b1 - b0)), dim3(256), 0, st, b0, b1, dnodes.as<NodeRec>(),
                                   dhas.as<uint8_t>());
                BCHK(hipGetLastError());
        }
        // the probes' side arrays: leaf lists at max depth, then their child
        // masks bottom-up; all zero when no probe reached a leaf
        const int nlevels = (int)out->level_begin.size() - 1;
        if (nprobe > 0) {
                BCHK(dpnode.alloc((size_t)nnodes * sizeof(uint2)));
                BCHK(hipMemsetAsync(dpnode, 0, (size_t)nnodes * sizeof(uint2), st));
        }
        if (nprefs > 0 && nlevels == D) {
                unsigned int *const lcnt = cnt.as<unsigned int>() + 2;
                BCHK(hipMemsetAsync(lcnt, 0, 4, st));
                BCHK(dpref.alloc((size_t)nprefs * 4));
                hipLaunchKernelGGL(k_pref, dim3(grid_of(nprefs)), dim3(256), 0, st, nprefs, pkeys_s.as<uint64_t>(),
                                   dpref.as<uint32_t>());
                BCHK(hipGetLastError());
                const int64_t b0 = out->level_begin[D - 1], b1 = out->level_begin[D];
                hipLaunchKernelGGL(k_probe_leaves, dim3(grid_of(b1 - b0)), dim3(256), 0, st, D, b0, b1 - b0,
                                   iall.as<uint32_t>(), pkeys_s.as<uint64_t>(), nprefs, dpnode.as<uint2>(), lcnt);
                BCHK(hipGetLastError());
                BCHK(dphas.alloc((size_t)nnodes));
                for (int l = nlevels; l >= 1; --l) {
                        const int64_t c0 = out->level_begin[l - 1], c1 = out->level_begin[l];
                        hipLaunchKernelGGL(k_probe_masks, dim3(grid_of(c1 - c0)), dim3(256), 0, st, c0, c1,
                                           dnodes.as<NodeRec>(), dpnode.as<uint2>(), dphas.as<uint8_t>());
                        BCHK(hipGetLastError());
                }
        }
        BCHK(hipEventRecord(e1, st));
        BCHK(hipEventSynchronize(e1));
        float ms = 0.f;
        BCHK(hipEventElapsedTime(&ms, e0, e1));
        out->device_ms = ms;
        out->ninternal = ninternal;
        out->nodes.resize((size_t)nnodes);
        out->node_vox.resize((size_t)nnodes);
        out->refs.resize((size_t)nrefs);
        BCHK(hipMemcpy(out->nodes.data(), dnodes, (size_t)nnodes * sizeof(NodeRec), hipMemcpyDeviceToHost));
        BCHK(hipMemcpy(out->node_vox.data(), dvox, (size_t)nnodes * 4, hipMemcpyDeviceToHost));
        if (nrefs)
                BCHK(hipMemcpy(out->refs.data(), keys_s, (size_t)nrefs * 8, hipMemcpyDeviceToHost));
        out->pnode.clear();
        out->pref.clear();
        out->probe_leaves = 0;
        if (nprobe > 0) {
                out->pnode.resize((size_t)nnodes);
                BCHK(hipMemcpy(out->pnode.data(), dpnode, (size_t)nnodes * sizeof(uint2), hipMemcpyDeviceToHost));
        }
        if (nprefs > 0 && nlevels == D) {
                unsigned int hl = 0;
                out->pref.resize((size_t)nprefs);
                BCHK(hipMemcpy(out->pref.data(), dpref, (size_t)nprefs * 4, hipMemcpyDeviceToHost));
                BCHK(hipMemcpy(&hl, cnt.as<unsigned int>() + 2, 4, hipMemcpyDeviceToHost));
                out->probe_leaves = hl;
        }
        return hipSuccess;
}

// Stable device radix sort of (uint32 key, uint32 value) pairs on the low
// `bits` key bits, for the light-map accumulation (vrt_kernels.hip: leaf
// key, canonical sample index); the same hipCUB / rocPRIM onesweep sort the
// build's frontier uses, so hipCUB's templates compile in this one file.
hipError_t sort_pairs_u64(void *temp, size_t *temp_bytes, const uint64_t *keys_in, uint64_t *keys_out,
                          const uint32_t *vals_in, uint32_t *vals_out, int64_t n, int bits, hipStream_t st)
{
        return hipcub::DeviceRadixSort::SortPairs(temp, *temp_bytes, keys_in, keys_out, vals_in, vals_out,
                                                  (int)n, 0, bits, st);
}

}  // namespace vrt
