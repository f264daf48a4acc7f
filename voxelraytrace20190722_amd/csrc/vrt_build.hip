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


// ---- scene update: root box and the finish of a build on the device -------
// (vrt_host.cpp's build_tree root merge, finish_tree, ref_boxes, march_nodes,
// chain_spacing and the TriPos / TriAttr fill, restated)

// Order-preserving map of a float's bits to uint32 (-0 folded onto +0).
__host__ __device__ __forceinline__ uint32_t ord_f32(float f)
{
        uint32_t u = __builtin_bit_cast(uint32_t, f);
        if (u == 0x80000000u)
                u = 0;
        return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// The same for a double, and back.
__host__ __device__ __forceinline__ uint64_t ord_f64(double d)
{
        const uint64_t u = __builtin_bit_cast(uint64_t, d);
        return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v)
{
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
                const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
                const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
                const uint64_t w = ((uint64_t)hi << 32) | lo;
                v = w < v ? w : v;
        }
        return v;
}

// keys[k] (min of axis k) and keys[3 + k] (max) start as all ones.  A key is
// (ordered value, or its complement for the max) << 32 | 3 * tri + vertex, so
// the smallest key is the extreme value's first occurrence in input order;
// only values below FLT_MAX (above -FLT_MAX) can replace the initial box,
// which leaves NaN out.
__global__ __launch_bounds__(256) void k_root_keys(int n, const float *__restrict__ pos,
                                                   unsigned long long *__restrict__ keys)
{
        const int i = blockIdx.x * blockDim.x + threadIdx.x;
        uint64_t mn[3] = { ~0ull, ~0ull, ~0ull }, mx[3] = { ~0ull, ~0ull, ~0ull };
        if (i < n) {
#pragma unroll
                for (int v = 0; v < 3; ++v)
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                                const float f = pos[9 * (int64_t)i + 3 * v + k];
                                const uint32_t seq = 3u * (uint32_t)i + (uint32_t)v;
                                if (f < kFltMax) {
                                        const uint64_t key = ((uint64_t)ord_f32(f) << 32) | seq;
                                        mn[k] = key < mn[k] ? key : mn[k];
                                }
                                if (f > -kFltMax) {
                                        const uint64_t key = ((uint64_t)(~ord_f32(f)) << 32) | seq;
                                        mx[k] = key < mx[k] ? key : mx[k];
                                }
                        }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
                const uint64_t a = wave_min_u64(mn[k]), b = wave_min_u64(mx[k]);
                if ((threadIdx.x & 63) == 0) {
                        if (a != ~0ull)
                                atomicMin(&keys[k], (unsigned long long)a);
                        if (b != ~0ull)
                                atomicMin(&keys[3 + k], (unsigned long long)b);
                }
        }
}

// The probes' faces behind the vertices (build_tree merges every probe's
// {o - r, o + r}, one float operation each, after the triangles and in probe
// order): probe i has sequence number seq0 + i, seq0 = 3 * ntri, so a vertex
// beats a probe face of the same value and probe i beats probe i + 1.  The
// probes are checked here as vrt_scene_create_probes checks them: *bad = the
// lowest index of a probe with a centre that is not finite or a radius that
// is not finite or negative (starts as all ones).
__global__ __launch_bounds__(256) void k_root_keys_probes(int n, const float4 *__restrict__ probes, uint32_t seq0,
                                                          unsigned long long *__restrict__ keys, unsigned int *bad)
{
        const int i = blockIdx.x * blockDim.x + threadIdx.x;
        uint64_t mn[3] = { ~0ull, ~0ull, ~0ull }, mx[3] = { ~0ull, ~0ull, ~0ull };
        if (i < n) {
                const float4 pb = probes[i];
                const float o[3] = { pb.x, pb.y, pb.z };
                const float inf = __builtin_huge_valf();
                const bool finite = fabsf(o[0]) < inf && fabsf(o[1]) < inf && fabsf(o[2]) < inf && fabsf(pb.w) < inf;
                if (!finite || pb.w < 0.f)
                        atomicMin(bad, (unsigned int)i);
                const uint32_t seq = seq0 + (uint32_t)i;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                        const float lo = o[k] - pb.w, hi = o[k] + pb.w;
                        if (lo < kFltMax)
                                mn[k] = ((uint64_t)ord_f32(lo) << 32) | seq;
                        if (hi > -kFltMax)
                                mx[k] = ((uint64_t)(~ord_f32(hi)) << 32) | seq;
                }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
                const uint64_t a = wave_min_u64(mn[k]), b = wave_min_u64(mx[k]);
                if ((threadIdx.x & 63) == 0) {
                        if (a != ~0ull)
                                atomicMin(&keys[k], (unsigned long long)a);
                        if (b != ~0ull)
                                atomicMin(&keys[3 + k], (unsigned long long)b);
                }
        }
}

// the float at each winning index (its own sign of zero); a sequence number
// from nvert = 3 * ntri on is a probe's face, computed again
__global__ void k_root_box(const float *__restrict__ pos, const float4 *__restrict__ probes, uint32_t nvert,
                           const unsigned long long *__restrict__ keys, float *__restrict__ box)
{
        const int j = threadIdx.x;
        if (j >= 6)
                return;
        const int k = j % 3;
        const uint64_t key = keys[j];
        if (key == ~0ull) {
                box[j] = j < 3 ? kFltMax : -kFltMax;
                return;
        }
        const uint32_t seq = (uint32_t)(key & 0xFFFFFFFFu);
        if (seq < nvert || !probes) {
                box[j] = pos[9 * (int64_t)(seq / 3u) + 3 * (seq % 3u) + k];
                return;
        }
        const float4 pb = probes[seq - nvert];
        const float o = k == 0 ? pb.x : k == 1 ? pb.y : pb.z;
        box[j] = j < 3 ? o - pb.w : o + pb.w;
}

__global__ __launch_bounds__(256) void k_leaf_counts(int64_t n, const NodeRec *__restrict__ nodes,
                                                     unsigned int *counts)
{
        const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        uint32_t leaf = 0, full = 0;
        if (i < n) {
                const uint32_t a = nodes[i].a;
                leaf = (a & kLeafBit) ? 1u : 0u;
                full = (leaf && (a & ~kLeafBit)) ? 1u : 0u;
        }
        (void)wave_append(leaf, counts);
        (void)wave_append(full, counts + 1);
}

// finish_tree's records from the sorted keys
__global__ __launch_bounds__(256) void k_leaf_records(int64_t n, const uint64_t *__restrict__ keys,
                                                      const float *__restrict__ pos, int wide, void *refs,
                                                      uint32_t *__restrict__ ref_tri)
{
        const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= n)
                return;
        const uint32_t t = (uint32_t)(keys[i] & 0xFFFFFFFFu);
        ref_tri[i] = t;
        const float *p = pos + 9 * (int64_t)t;
        if (wide) {
                RefRec64 rr;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                        rr.v0[k] = p[k];
                        rr.e1[k] = (double)p[3 + k] - (double)p[k];
                        rr.e2[k] = (double)p[6 + k] - (double)p[k];
                }
                rr.tri = t;
                static_cast<RefRec64 *>(refs)[i] = rr;
        } else {
                RefRec48 rr;
#pragma unroll
                for (int k = 0; k < 9; ++k)
                        rr.p[k] = p[k];
                rr.tri = t;
                rr.pad[0] = rr.pad[1] = 0;
                static_cast<RefRec48 *>(refs)[i] = rr;
        }
}

// std::min / std::max of doubles as the host loops use them
__device__ __forceinline__ double dmin(double a, double b) { return (b < a) ? b : a; }
__device__ __forceinline__ double dmax(double a, double b) { return (a < b) ? b : a; }

// std::nextafter(f, -inf) / (f, +inf) for the values enlarged_box steps
__device__ __forceinline__ float step_down(float f)
{
        uint32_t u = __builtin_bit_cast(uint32_t, f);
        if (f != f || u == 0xFF800000u)
                return f;
        if ((u & 0x7FFFFFFFu) == 0)
                u = 0x80000001u;
        else
                u = (u & 0x80000000u) ? u + 1 : u - 1;
        return __builtin_bit_cast(float, u);
}
__device__ __forceinline__ float step_up(float f)
{
        uint32_t u = __builtin_bit_cast(uint32_t, f);
        if (f != f || u == 0x7F800000u)
                return f;
        if ((u & 0x7FFFFFFFu) == 0)
                u = 0x00000001u;
        else
                u = (u & 0x80000000u) ? u - 1 : u + 1;
        return __builtin_bit_cast(float, u);
}
// enlarged_box (vrt_host.cpp)
__device__ __forceinline__ void enlarged_box_dev(const double *l, const double *h, double eps, float *bl, float *bh)
{
#pragma unroll
        for (int k = 0; k < 3; ++k) {
                float fl = (float)(l[k] - eps), fh = (float)(h[k] + eps);
                if ((double)fl > l[k] - eps)
                        fl = step_down(fl);
                if ((double)fh < h[k] + eps)
                        fh = step_up(fh);
                bl[k] = fl;
                bh[k] = fh;
        }
}

// ref_boxes: record j's box at ((RefBox *)refs)[-1 - j]
__global__ __launch_bounds__(256) void k_ref_boxes(int64_t n, const uint32_t *__restrict__ ref_tri,
                                                   const float *__restrict__ pos, double eps, void *refs)
{
        const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (j >= n)
                return;
        const float *p = pos + 9 * (int64_t)ref_tri[j];
        const double inf = __builtin_huge_val();
        double l[3] = { inf, inf, inf }, h[3] = { -inf, -inf, -inf };
        bool nan = false;
#pragma unroll
        for (int v = 0; v < 3; ++v)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                        const float f = p[3 * v + k];
                        nan = nan || f != f;
                        l[k] = dmin(l[k], (double)f);
                        h[k] = dmax(h[k], (double)f);
                }
        RefBox rb{};
        if (nan) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                        rb.bmin[k] = __builtin_huge_valf();
                        rb.bmax[k] = -__builtin_huge_valf();
                }
        } else {
                enlarged_box_dev(l, h, eps, rb.bmin, rb.bmax);
        }
        static_cast<RefBox *>(refs)[-1 - j] = rb;
}

// march_nodes: the node record and its voxel box
__global__ __launch_bounds__(256) void k_xnode_init(int64_t n, const NodeRec *__restrict__ nodes,
                                                    XNodeRec *__restrict__ xn)
{
        const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= n)
                return;
        XNodeRec x;
        x.n = nodes[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
                x.tmin[k] = x.n.bmin[k];
                x.tmax[k] = x.n.bmax[k];
        }
        x.pad[0] = x.pad[1] = 0;
        xn[i] = x;
}

// the unenlarged triangle union boxes of one level (the levels below are done):
// lohi[6i .. 6i+2] = lo, [6i+3 .. 6i+5] = hi
__global__ __launch_bounds__(256) void k_xnode_level(int64_t begin, int64_t end, const NodeRec *__restrict__ nodes,
                                                     const uint32_t *__restrict__ ref_tri,
                                                     const float *__restrict__ pos, double *__restrict__ lohi)
{
        const int64_t i = begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= end)
                return;
        const NodeRec nr = nodes[i];
        const double inf = __builtin_huge_val();
        double l[3] = { inf, inf, inf }, h[3] = { -inf, -inf, -inf };
        if (nr.a & kLeafBit) {
                const uint32_t n = nr.a & ~kLeafBit;
                for (uint32_t j = 0; j < n; ++j) {
                        const float *p = pos + 9 * (int64_t)ref_tri[nr.b + j];
                        for (int v = 0; v < 3; ++v)
#pragma unroll
                                for (int k = 0; k < 3; ++k) {
                                        l[k] = dmin(l[k], (double)p[3 * v + k]);
                                        h[k] = dmax(h[k], (double)p[3 * v + k]);
                                }
                }
        } else {
                for (uint32_t c = 0; c < 8; ++c) {
                        const double *cl = lohi + 6 * (int64_t)(nr.a + c);
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                                l[k] = dmin(l[k], cl[k]);
                                h[k] = dmax(h[k], cl[3 + k]);
                        }
                }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
                lohi[6 * i + k] = l[k];
                lohi[6 * i + 3 + k] = h[k];
        }
}

__global__ __launch_bounds__(256) void k_xnode_enlarge(int64_t n, const double *__restrict__ lohi, double eps,
                                                       XNodeRec *__restrict__ xn)
{
        const int64_t i = 1 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= n)
                return;
        const double *l = lohi + 6 * i, *h = l + 3;
        if (!(l[0] <= h[0]))
                return;  // no triangle below this node
        enlarged_box_dev(l, h, eps, xn[i].tmin, xn[i].tmax);
}

// chain_spacing's loop over the internal nodes: out[k] = the ordered key of
// min (double)c1 - (double)c0 of axis k (all ones: none), out[3] != 0: some
// centre lies outside the root box or is NaN
__global__ __launch_bounds__(256) void k_chain(int64_t n, const NodeRec *__restrict__ nodes,
                                               unsigned long long *__restrict__ out)
{
        const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        uint64_t w[3] = { ~0ull, ~0ull, ~0ull };
        bool ok = true;
        if (i < n) {
                const NodeRec nr = nodes[i];
                if (!(nr.a & kLeafBit)) {
                        const NodeRec root = nodes[0];
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                                const float h = (nr.bmax[k] - nr.bmin[k]) / 2.0f;
                                const float a0 = nr.bmin[k];
                                const float b = nr.bmin[k] + h;
                                const float c = b + h;
                                const float c0 = (a0 + b) * .5f;
                                const float c1 = (b + c) * .5f;
                                const double d = (double)c1 - (double)c0;
                                if (d == d)  // std::min(w, NaN) keeps w
                                        w[k] = ord_f64(d);
                                ok = ok && c0 >= root.bmin[k] && c0 <= root.bmax[k] && c1 >= root.bmin[k] &&
                                     c1 <= root.bmax[k];
                        }
                }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
                const uint64_t a = wave_min_u64(w[k]);
                if ((threadIdx.x & 63) == 0 && a != ~0ull)
                        atomicMin(&out[k], (unsigned long long)a);
        }
        if (!ok)
                out[3] = 1ull;
}

// TriPos, and TriAttr's normals (Triangle::Triangle's normalize); uv and
// material stay
__global__ __launch_bounds__(256) void k_tri_tables(int n, const float *__restrict__ pos,
                                                    const float *__restrict__ nrm, TriPos *__restrict__ tp,
                                                    TriAttr *__restrict__ ta)
{
        const int i = blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= n)
                return;
        TriPos t;
#pragma unroll
        for (int k = 0; k < 9; ++k)
                t.p[k] = pos[9 * (int64_t)i + k];
        t.pad[0] = t.pad[1] = t.pad[2] = 0.f;
        tp[i] = t;
        if (nrm) {
#pragma unroll
                for (int v = 0; v < 3; ++v) {
                        const float *nn = nrm + 9 * (int64_t)i + 3 * v;
                        const f3 q = normalize(mk3(nn[0], nn[1], nn[2]));
                        ta[i].n[3 * v + 0] = q.x;
                        ta[i].n[3 * v + 1] = q.y;
                        ta[i].n[3 * v + 2] = q.z;
                }
        }
}

unsigned grid_of(int64_t n)
{
        return (unsigned)((n + 255) / 256);
}

}  // namespace

// A copy the host waits for: on the null stream as the build always made it,
// on a stream of its own in that stream's order (after which a host source is
// the caller's again).
static hipError_t copy_sync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t st)
{
        if (!st)
                return hipMemcpy(dst, src, bytes, kind);
        if (hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, st))
                return e;
        return hipStreamSynchronize(st);
}
// a counter the host needs
static hipError_t read_word(void *dst, const void *src, hipStream_t st)
{
        return copy_sync(dst, src, 4, hipMemcpyDeviceToHost, st);
}

hipError_t build_frontier_device(BuildScratch &sc, const float *d_pos, int ntri, const float root_mn[3],
                                 const float root_mx[3], int D, const float4 *d_probes, int nprobe, hipStream_t st,
                                 bool fail_limit, DeviceTree *out, std::string *err)
{
        GrowMem &cnt = sc.cnt, &pa = sc.pa, &pb = sc.pb, &codes = sc.codes, &codes_s = sc.codes_s, &uniq = sc.uniq,
                &nuniq = sc.nuniq, &temp = sc.temp, &iall = sc.iall, &keys = sc.keys, &keys_s = sc.keys_s,
                &inode = sc.inode, &dnodes = sc.nodes, &dvox = sc.vox, &dhas = sc.has;
        // the probe frontier and its outputs
        GrowMem &qa = sc.qa, &qb = sc.qb, &pkeys = sc.pkeys, &pkeys_s = sc.pkeys_s, &dpref = sc.pref,
                &dpnode = sc.pnode, &dphas = sc.phas;
        BCHK(cnt.need(16));
        Pair root;
        for (int k = 0; k < 3; ++k) {
                root.mn[k] = root_mn[k];
                root.mx[k] = root_mx[k];
        }
        root.tri = 0;
        root.code = 0;
        // level 1 frontier
        BCHK(pa.need((size_t)std::max(1, ntri) * sizeof(Pair)));
        BCHK(hipMemsetAsync(cnt, 0, 16, st));
        if (ntri > 0)
                hipLaunchKernelGGL(k_seed, dim3(grid_of(ntri)), dim3(256), 0, st, ntri, d_pos, root,
                                   pa.as<Pair>(), cnt.as<unsigned int>());
        BCHK(hipGetLastError());
        unsigned int hn = 0;
        BCHK(read_word(&hn, cnt, st));
        int64_t n = hn;
        // the probes' counter is the second word of cnt
        unsigned int *const qcnt = cnt.as<unsigned int>() + 1;
        int64_t nq = 0;
        if (nprobe > 0) {
                BCHK(qa.need((size_t)nprobe * sizeof(Pair)));
                hipLaunchKernelGGL(k_seed_probes, dim3(grid_of(nprobe)), dim3(256), 0, st, nprobe,
                                   d_probes, root, qa.as<Pair>(), qcnt);
                BCHK(hipGetLastError());
                BCHK(read_word(&hn, qcnt, st));
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
                                BCHK(pkeys.need((size_t)nq * 8));
                                BCHK(pkeys_s.need((size_t)nq * 8));
                                hipLaunchKernelGGL(k_leaf_keys, dim3(grid_of(nq)), dim3(256), 0, st, nq, qa.as<Pair>(),
                                                   pkeys.as<uint64_t>());
                                BCHK(hipGetLastError());
                                size_t tb = 0;
                                const int bits = 32 + 3 * (D - 1);
                                BCHK(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, pkeys.as<uint64_t>(),
                                                                       pkeys_s.as<uint64_t>(), (int)nq, 0, bits, st));
                                BCHK(temp.need(tb));
                                BCHK(hipcub::DeviceRadixSort::SortKeys(temp, tb, pkeys.as<uint64_t>(),
                                                                       pkeys_s.as<uint64_t>(), (int)nq, 0, bits, st));
                        }
                        // leaf lists: sort (code << 32 | tri)
                        nrefs = n;
                        BCHK(keys.need((size_t)std::max<int64_t>(1, n) * 8));
                        BCHK(keys_s.need((size_t)std::max<int64_t>(1, n) * 8));
                        if (n > 0) {
                                hipLaunchKernelGGL(k_leaf_keys, dim3(grid_of(n)), dim3(256), 0, st, n, pa.as<Pair>(),
                                                   keys.as<uint64_t>());
                                BCHK(hipGetLastError());
                                size_t tb = 0;
                                const int bits = 32 + 3 * (D - 1);
                                BCHK(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, keys.as<uint64_t>(),
                                                                       keys_s.as<uint64_t>(), (int)n, 0, bits, st));
                                BCHK(temp.need(tb));
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
                BCHK(codes.need((size_t)std::max<int64_t>(1, nc) * 4));
                BCHK(pb.need((size_t)std::max<int64_t>(1, 8 * n) * sizeof(Pair)));
                BCHK(hipMemsetAsync(cnt, 0, 16, st));
                if (n > 0)
                        hipLaunchKernelGGL(k_expand, dim3(grid_of(n)), dim3(256), 0, st, n, pa.as<Pair>(),
                                           d_pos, codes.as<uint32_t>(), pb.as<Pair>(),
                                           cnt.as<unsigned int>());
                BCHK(hipGetLastError());
                if (nq > 0) {
                        BCHK(qb.need((size_t)(8 * nq) * sizeof(Pair)));
                        hipLaunchKernelGGL(k_expand_probes, dim3(grid_of(nq)), dim3(256), 0, st, nq, qa.as<Pair>(),
                                           d_probes, codes.as<uint32_t>() + n, qb.as<Pair>(), qcnt);
                        BCHK(hipGetLastError());
                }
                // internal nodes of level l = sorted unique codes
                int64_t nu = 0;
                if (nc > 0) {
                        const int bits = std::max(1, 3 * (l - 1));
                        BCHK(codes_s.need((size_t)nc * 4));
                        BCHK(uniq.need((size_t)nc * 4));
                        BCHK(nuniq.need(8));
                        size_t tb = 0, tb2 = 0;
                        BCHK(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, codes.as<uint32_t>(), codes_s.as<uint32_t>(),
                                                               (int)nc, 0, bits, st));
                        BCHK(hipcub::DeviceSelect::Unique(nullptr, tb2, codes_s.as<uint32_t>(), uniq.as<uint32_t>(),
                                                          nuniq.as<int>(), (int)nc, st));
                        BCHK(temp.need(std::max(tb, tb2)));
                        BCHK(hipcub::DeviceRadixSort::SortKeys(temp, tb, codes.as<uint32_t>(), codes_s.as<uint32_t>(),
                                                               (int)nc, 0, bits, st));
                        BCHK(hipcub::DeviceSelect::Unique(temp, tb2, codes_s.as<uint32_t>(), uniq.as<uint32_t>(),
                                                          nuniq.as<int>(), (int)nc, st));
                        int hnu = 0;
                        BCHK(read_word(&hnu, nuniq, st));
                        nu = hnu;
                        const size_t o = h_iall.size();
                        h_iall.resize(o + (size_t)nu);
                        if (nu)
                                BCHK(copy_sync(h_iall.data() + o, uniq, (size_t)nu * 4, hipMemcpyDeviceToHost, st));
                }
                n_int[l] = nu;
                BCHK(read_word(&hn, cnt, st));
                n = hn;
                std::swap(pa, pb);
                if (nq > 0) {
                        BCHK(read_word(&hn, qcnt, st));
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
        BLIMIT(fail_limit, "octree too large (%lld nodes; VRT_TEST_UPDATE_TOO_LARGE)", (long long)nnodes);
        out->level_begin.clear();
        BCHK(iall.need(std::max<size_t>(1, h_iall.size()) * 4));
        if (!h_iall.empty())
                BCHK(copy_sync(iall, h_iall.data(), h_iall.size() * 4, hipMemcpyHostToDevice, st));
        BCHK(inode.need(std::max<int64_t>(1, ninternal) * 4));
        BCHK(dnodes.need((size_t)nnodes * sizeof(NodeRec)));
        BCHK(dvox.need((size_t)nnodes * 4));
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
        BCHK(dhas.need((size_t)nnodes));
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
                BCHK(dpnode.need((size_t)nnodes * sizeof(uint2)));
                BCHK(hipMemsetAsync(dpnode, 0, (size_t)nnodes * sizeof(uint2), st));
        }
        if (nprefs > 0 && nlevels == D) {
                unsigned int *const lcnt = cnt.as<unsigned int>() + 2;
                BCHK(hipMemsetAsync(lcnt, 0, 4, st));
                BCHK(dpref.need((size_t)nprefs * 4));
                hipLaunchKernelGGL(k_pref, dim3(grid_of(nprefs)), dim3(256), 0, st, nprefs, pkeys_s.as<uint64_t>(),
                                   dpref.as<uint32_t>());
                BCHK(hipGetLastError());
                const int64_t b0 = out->level_begin[D - 1], b1 = out->level_begin[D];
                hipLaunchKernelGGL(k_probe_leaves, dim3(grid_of(b1 - b0)), dim3(256), 0, st, D, b0, b1 - b0,
                                   iall.as<uint32_t>(), pkeys_s.as<uint64_t>(), nprefs, dpnode.as<uint2>(), lcnt);
                BCHK(hipGetLastError());
                BCHK(dphas.need((size_t)nnodes));
                for (int l = nlevels; l >= 1; --l) {
                        const int64_t c0 = out->level_begin[l - 1], c1 = out->level_begin[l];
                        hipLaunchKernelGGL(k_probe_masks, dim3(grid_of(c1 - c0)), dim3(256), 0, st, c0, c1,
                                           dnodes.as<NodeRec>(), dpnode.as<uint2>(), dphas.as<uint8_t>());
                        BCHK(hipGetLastError());
                }
        }
        out->nodes = dnodes.as<NodeRec>();
        out->node_vox = dvox.as<uint32_t>();
        out->refs = keys_s.as<uint64_t>();
        out->nnodes = nnodes;
        out->nrefs = nrefs;
        out->ninternal = ninternal;
        out->pnode = nprobe > 0 ? dpnode.as<uint2>() : nullptr;
        out->pref = nullptr;
        out->nprefs = 0;
        out->probe_leaves = nullptr;
        if (nprefs > 0 && nlevels == D) {
                out->pref = dpref.as<uint32_t>();
                out->nprefs = nprefs;
                out->probe_leaves = cnt.as<unsigned int>() + 2;
        }
        return hipSuccess;
}

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
        BuildScratch sc;
        GrowMem &dpos = sc.pos, &dprobes = sc.nrm;
        BCHK(dpos.need((size_t)ntri * 36));
        BCHK(hipMemcpy(dpos, pos, (size_t)ntri * 36, hipMemcpyHostToDevice));
        if (nprobe > 0) {
                BCHK(dprobes.need((size_t)nprobe * sizeof(float4)));
                BCHK(hipMemcpy(dprobes, probes, (size_t)nprobe * sizeof(float4), hipMemcpyHostToDevice));
        }
        BCHK(hipEventRecord(e0, st));
        DeviceTree t;
        const hipError_t fe = build_frontier_device(sc, dpos.as<float>(), ntri, root_mn, root_mx, D,
                                                    dprobes.as<float4>(), nprobe, st, false, &t, err);
        if (fe != hipSuccess) {
                out->too_large = t.too_large;
                return fe;
        }
        const int64_t nnodes = t.nnodes, nrefs = t.nrefs;
        BCHK(hipEventRecord(e1, st));
        BCHK(hipEventSynchronize(e1));
        float ms = 0.f;
        BCHK(hipEventElapsedTime(&ms, e0, e1));
        out->device_ms = ms;
        out->ninternal = t.ninternal;
        out->level_begin = t.level_begin;
        out->nodes.resize((size_t)nnodes);
        out->node_vox.resize((size_t)nnodes);
        out->refs.resize((size_t)nrefs);
        BCHK(hipMemcpy(out->nodes.data(), t.nodes, (size_t)nnodes * sizeof(NodeRec), hipMemcpyDeviceToHost));
        BCHK(hipMemcpy(out->node_vox.data(), t.node_vox, (size_t)nnodes * 4, hipMemcpyDeviceToHost));
        if (nrefs)
                BCHK(hipMemcpy(out->refs.data(), t.refs, (size_t)nrefs * 8, hipMemcpyDeviceToHost));
        out->pnode.clear();
        out->pref.clear();
        out->probe_leaves = 0;
        if (nprobe > 0) {
                out->pnode.resize((size_t)nnodes);
                BCHK(hipMemcpy(out->pnode.data(), t.pnode, (size_t)nnodes * sizeof(uint2), hipMemcpyDeviceToHost));
        }
        if (t.nprefs > 0) {
                unsigned int hl = 0;
                out->pref.resize((size_t)t.nprefs);
                BCHK(hipMemcpy(out->pref.data(), t.pref, (size_t)t.nprefs * 4, hipMemcpyDeviceToHost));
                BCHK(hipMemcpy(&hl, t.probe_leaves, 4, hipMemcpyDeviceToHost));
                out->probe_leaves = hl;
        }
        return hipSuccess;
}

hipError_t launch_root_box(const float *d_pos, int ntri, const float4 *d_probes, int nprobe, uint64_t *keys,
                           float *box, hipStream_t st)
{
        if (hipError_t e = hipMemsetAsync(keys, 0xFF, 6 * sizeof(uint64_t), st))
                return e;
        if (ntri > 0)
                hipLaunchKernelGGL(k_root_keys, dim3(grid_of(ntri)), dim3(256), 0, st, ntri, d_pos,
                                   reinterpret_cast<unsigned long long *>(keys));
        if (nprobe > 0) {
                unsigned int *const bad = reinterpret_cast<unsigned int *>(box + 6);
                if (hipError_t e = hipMemsetAsync(bad, 0xFF, sizeof *bad, st))
                        return e;
                hipLaunchKernelGGL(k_root_keys_probes, dim3(grid_of(nprobe)), dim3(256), 0, st, nprobe, d_probes,
                                   3u * (uint32_t)ntri, reinterpret_cast<unsigned long long *>(keys), bad);
        }
        hipLaunchKernelGGL(k_root_box, dim3(1), dim3(64), 0, st, d_pos, nprobe > 0 ? d_probes : nullptr,
                           3u * (uint32_t)ntri, reinterpret_cast<const unsigned long long *>(keys), box);
        return hipGetLastError();
}

hipError_t launch_leaf_counts(const NodeRec *nodes, int64_t n, unsigned int *counts, hipStream_t st)
{
        if (hipError_t e = hipMemsetAsync(counts, 0, 8, st))
                return e;
        hipLaunchKernelGGL(k_leaf_counts, dim3(grid_of(n)), dim3(256), 0, st, n, nodes, counts);
        return hipGetLastError();
}

double chain_key_value(uint64_t key)
{
        const uint64_t u = (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key;
        return __builtin_bit_cast(double, u);
}

hipError_t launch_finish(const FinishArgs &a, hipStream_t st)
{
        const DeviceTree &t = *a.tree;
        if (t.nrefs > 0) {
                hipLaunchKernelGGL(k_leaf_records, dim3(grid_of(t.nrefs)), dim3(256), 0, st, t.nrefs, t.refs, a.pos,
                                   a.wide, a.refs, a.ref_tri);
                if (a.rboxes)
                        hipLaunchKernelGGL(k_ref_boxes, dim3(grid_of(t.nrefs)), dim3(256), 0, st, t.nrefs,
                                           (const uint32_t *)a.ref_tri, a.pos, a.eps, a.refs);
        }
        hipLaunchKernelGGL(k_xnode_init, dim3(grid_of(t.nnodes)), dim3(256), 0, st, t.nnodes, t.nodes, a.xnodes);
        if (a.lb_on) {
                for (int l = (int)t.level_begin.size() - 1; l >= 1; --l) {
                        const int64_t b0 = t.level_begin[l - 1], b1 = t.level_begin[l];
                        if (b1 > b0)
                                hipLaunchKernelGGL(k_xnode_level, dim3(grid_of(b1 - b0)), dim3(256), 0, st, b0, b1,
                                                   t.nodes, (const uint32_t *)a.ref_tri, a.pos, a.lohi);
                }
                if (t.nnodes > 1)
                        hipLaunchKernelGGL(k_xnode_enlarge, dim3(grid_of(t.nnodes - 1)), dim3(256), 0, st, t.nnodes,
                                           (const double *)a.lohi, a.eps, a.xnodes);
        }
        if (a.chain) {
                if (hipError_t e = hipMemsetAsync(a.chain_out, 0xFF, 24, st))
                        return e;
                if (hipError_t e = hipMemsetAsync(a.chain_out + 3, 0, 8, st))
                        return e;
                hipLaunchKernelGGL(k_chain, dim3(grid_of(t.nnodes)), dim3(256), 0, st, t.nnodes, t.nodes,
                                   reinterpret_cast<unsigned long long *>(a.chain_out));
        }
        if (a.ntri > 0)
                hipLaunchKernelGGL(k_tri_tables, dim3(grid_of(a.ntri)), dim3(256), 0, st, a.ntri, a.pos, a.nrm,
                                   a.tri_pos, a.tri_attr);
        return hipGetLastError();
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
