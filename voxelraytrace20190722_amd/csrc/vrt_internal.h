// vrt_internal.h -- device data layout shared by the host library and the
// gfx950 kernels.  See DESIGN.md "Data layout in HBM".
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <string>
#include <vector>

#include "vrt.h"
#include "vrt_math.h"

namespace vrt {

// One octree node, 32 B (two dwordx4 loads).  The 8 children of an internal
// node are contiguous.  Boxes are the exact float boxes split() produces
// (VRT/voxel_octree.cc:27-39).
//   internal:        a = index of first child      (bit 31 clear)
//   leaf:            a = kLeafBit | triangle count, b = first ref record
struct alignas(16) NodeRec {
        float bmin[3];
        float bmax[3];
        uint32_t a;
        uint32_t b;
};
static_assert(sizeof(NodeRec) == 32, "NodeRec must be 32 B");
constexpr uint32_t kLeafBit = 0x80000000u;

// March record of the node triangle-box walk (DevScene::xnodes): the node's
// own record (voxel box, a, b) followed by the union box of every triangle
// below it (a leaf: its own triangles), enlarged by lb_eps -- one 64-B
// record, so the walk fetches both halves with one address.
struct alignas(16) XNodeRec {
        NodeRec n;
        float tmin[3];
        float tmax[3];
        uint32_t pad[2];
};
static_assert(sizeof(XNodeRec) == 64, "XNodeRec must be 64 B");


// Leaf-list records, in leaf order with the vertices inlined (no dependent
// index load in the leaf loop).  Two formats, chosen per scene:
// RefRec48 for small leaves (fewer bytes per gather), RefRec64 for scenes
// with >= 8 records per non-empty leaf (DevScene::wide_leaves), where the
// leaf loop dominates and a wave often tests one leaf together.
struct alignas(16) RefRec48 {
        float p[9];
        uint32_t tri;
        uint32_t pad[2];
};
static_assert(sizeof(RefRec48) == 48, "RefRec48 must be 48 B");
// 64 B (one cache line): vert0 as float (widened in the kernel), the
// triangle id, and Moller-Trumbore's edge1 = vert1 - vert0, edge2 = vert2 -
// vert0 already in double -- the same IEEE subtractions of widened floats
// intersect_triangle3 makes (VRT/raytri.cc:209-210), done once per record.
struct alignas(16) RefRec64 {
        float v0[3];
        uint32_t tri;
        double e1[3];
        double e2[3];
};
static_assert(sizeof(RefRec64) == 64, "RefRec64 must be 64 B");

// Leaf-record cull of the finite-slab walk (VRT_LEAF_CULL, RefRec48 scenes):
// one box per leaf record -- record j's triangle's box enlarged by lb_eps and
// rounded outward, the box march_nodes gives a one-triangle leaf (both come
// from enlarged_box(), vrt_host.cpp) -- so a leaf's records are first tested
// by the fp32 line test on dense, independently loadable boxes and only the
// survivors take the dependent 48-B load and the fp64 triangle test.  A
// record whose box the line misses is one intersect_triangle3 rejects
// (DevScene::xnodes' argument for a single triangle), and survivors are
// tested in leaf order, so ray_march_isect's first minimum is unchanged.
// The array lies directly below DevScene::refs and grows downward: record
// j's box is ((const RefBox *)refs)[-1 - j].  No pointer is added to
// DevScene, so its layout -- and the code of every kernel that does not
// cull -- stays as it was.  Built only for RefRec48 scenes with lb_reach >=
// 0 (lanes cull only under leaf_box_ok, which lb_reach < 0 never grants).
// VRT_LEAF_CULL_BOX: bytes per box, 32 (two 16-B loads) or 24 (three 8-B
// loads); see DESIGN.md appendix for the A/B.
#ifndef VRT_LEAF_CULL
#define VRT_LEAF_CULL 1
#endif
#ifndef VRT_LEAF_CULL_BOX
#define VRT_LEAF_CULL_BOX 24
#endif
static_assert(VRT_LEAF_CULL_BOX == 24 || VRT_LEAF_CULL_BOX == 32, "VRT_LEAF_CULL_BOX");
struct alignas(VRT_LEAF_CULL_BOX == 32 ? 16 : 8) RefBox {
        float bmin[3];
        float bmax[3];
#if VRT_LEAF_CULL_BOX == 32
        uint32_t pad[2];
#endif
};
static_assert(sizeof(RefBox) == VRT_LEAF_CULL_BOX, "RefBox size");
// Spare boxes below the last record's: the cull loop loads a leaf's boxes in
// groups and a group may run past the last leaf's end (never used, only
// loaded), so the array is allocated with this many more.
constexpr int kRefBoxPad = 7;

// Shading attributes of one triangle (64 B): normalised vertex normals
// (Triangle::Triangle, VRT/voxel_octree.cc:426), uvs, material id.
struct alignas(16) TriAttr {
        float n[9];
        float t[6];
        int32_t mat;
};
static_assert(sizeof(TriAttr) == 64, "TriAttr must be 64 B");

struct alignas(16) TriPos {
        float p[9];
        float pad[3];
};

struct alignas(16) TexRec {
        int64_t off;
        int32_t w, h, c, pad;
};

// A material with its texture's record inline (a copy of texs[tex]), so a
// textured hit's shading is TriAttr (beside TriPos) -> MatRec -> texel: one
// dependent load fewer than MatRec -> TexRec.
struct alignas(16) MatRec {
        int32_t tex;  // -1 = untextured: Kd
        float kd[3];
        TexRec tx;    // texs[tex] when tex >= 0, else zero
};
static_assert(sizeof(MatRec) == 48, "MatRec must be 48 B");

// Device-side scene view passed by value to kernels.
struct DevScene {
        const NodeRec *nodes;
        const uint32_t *node_vox;
        const void *refs;  // RefRec64 if wide_leaves, else RefRec48
        const TriPos *tri_pos;
        const TriAttr *tri_attr;
        const MatRec *mats;
        const TexRec *texs;
        const uint8_t *tex_data;
        int32_t max_depth;
        int32_t nmat, ntex;
        int32_t fast_ok;  // root box finite and |coords| < 2^60 (expand_v1, fast_ok())
        int32_t wide_leaves;  // >= 8 records per non-empty leaf on average: RefRec64 records,
                              // wave-uniform leaf loads (leaf_isect)
        int32_t persist_blocks;  // resident 256-thread blocks of the persistent render on this
                                 // device (a multiple of 8), 0 = no persistent launches
        int32_t sec_blocks;      // the same for the persistent secondary-ray kernel
        int32_t grid_div;        // persistent render grid = resident slots / grid_div
                                 // (vrt_scene_set_frames_in_flight)
        // March records of the nodes (XNodeRec): the node record and the
        // union box of every triangle below it enlarged by lb_eps
        // (leaf_box_ok).  A ray whose line misses that box cannot pass
        // intersect_triangle3 (which accepts a hit at any t) on any triangle
        // below the node, so the finite-slab walks skip the subtree (a leaf:
        // its triangle loop); results are unchanged.  The skip is used for
        // rays with every |o - lb_center| <= lb_reach, where lb_eps exceeds
        // the fp32 rounding of the line test.
        const XNodeRec *xnodes;
        float lb_center[3];
        float lb_reach;
};

// Work queue of one persistent launch (k_render_p, k_secondary_p): 8
// counters, one per XCD slice of the units, one 128-B line each.  The
// kernel never resets them: unit j of slice x is taken by the atomicAdd that
// returns base[x] + j, and every wave makes exactly one more (failing) add
// per non-empty slice, so after a launch of `waves` waves counter x has
// advanced by (hi - lo of queue_range(units, x)) + waves -- the host keeps
// base[] from that, per ring slot (vrt_host.cpp: queue_take /
// queue_release).  Launches on different streams use different slots; a
// slot is reused only after its previous launch has finished (an event), so
// no two launches share counters and no memset is needed.
// After the counters: the deferred-unit lists of k_render_p<true>, one per
// XCD slice (a wave appends a unit to the list of the slice it took it
// from; 8 counters instead of one keep the appends as spread as the takes):
// slice x's count at defer[x * kQueueStride + kDeferCount], its list at
// defer[kDeferList + x * kDeferSliceCap ...].  A slice with more than
// kDeferSliceCap deferred units is re-rendered whole.  k_render_defer,
// launched behind it on the same stream, renders them (its waves take
// entries from the slice's defer[x * kQueueStride + kDeferTake] and count
// themselves out on defer[kDeferDoneWord]); its last wave zeroes every count,
// take counter and the done counter.
constexpr int kQueueStride = 32;
constexpr int kQueueSlots = 8;
constexpr int kDeferCount = 0;
constexpr int kDeferTake = 1;
constexpr int kDeferDoneWord = 8 * kQueueStride;
constexpr int kDeferList = kDeferDoneWord + kQueueStride;
constexpr int kDeferSliceCap = 512;
constexpr size_t kQueueWords = 8 * kQueueStride + kDeferList + 8 * kDeferSliceCap;
constexpr size_t kQueueBytes = kQueueWords * sizeof(uint32_t);
struct WorkQueue {
        uint32_t *ctr;
        uint32_t *defer;
        uint32_t base[8];
};
// Beam entry of the persistent fast-only render (VRT_BEAM_ENTRY, DESIGN
// §4.2): before k_render_p<true>, k_unit_entry walks the octree once per unit
// (a unit's 64 rays share the origin) while every decision is certain for all
// 64 rays, and records the walk's loop-top state where it stops; the unit's
// wave starts there.  One record per unit, 64 B, one buffer per WorkQueue
// ring slot (vrt_scene::d_entry):
//   word 0: kEntryNone ("no entry": the wave runs its own prologue), else
//           the number of stack entries (0: no ray of the unit can hit) |
//           kEntryChainBit when every ray passes chain_criterion
//   words 2 + 2i, 3 + 2i: stack entry i < kEntryMax in ray_march's format
//           (base, order | cnt << 24), cnt > 0; the level being walked is the
//           top entry
#ifndef VRT_BEAM_ENTRY
#define VRT_BEAM_ENTRY 1
#endif
constexpr int kEntryWords = 16;
constexpr int kEntryMax = 7;
constexpr uint32_t kEntryNone = 0xFFFFFFFFu;
constexpr uint32_t kEntryCountMask = 0xFFu;
constexpr uint32_t kEntryChainBit = 0x100u;
// Smallest one-rank frame that takes the entry.  The pre-pass is one long
// dependent chain per lane (64 rays, then ~10 visits), whatever the size,
// against a quarter of the render's time saved.  Measured with 3 frames in
// flight, without -> with the entry: 8,160 units 0.180 -> 0.216 ms per frame
// and 129,600 units 0.86 -> 0.72 with the first pre-pass; 32,640 units
// (960x544) 0.310 -> 0.312 with it and 0.3173 -> 0.3023 with the present one
// (115 instead of 190 VALU per ray), whose margin of 0.010 ms exceeds the
// spread of 0.007: the limit is that frame's size, the smallest measured to
// win.  VRT_TEST_SMALL_BEAM_ENTRY lifts the limit.
constexpr int64_t kEntryMinUnits = 32640;
// units of slice x: a contiguous range [lo, hi) of the unit order
__host__ __device__ inline void queue_range(int units, int x, int &lo, int &hi)
{
        const int per = (units + 7) >> 3;
        lo = x * per;
        hi = lo + per < units ? lo + per : units;
        if (hi < lo)
                hi = lo;
}

// XCD slices of a persistent launch's units (the kernels and the host's
// queue bases agree through these two functions).  ch = 0: slice x is
// queue_range's contiguous eighth of the units; ch > 0: the unit order is cut
// into chunks of ch units dealt to the slices round-robin (chunk c -> slice c
// % 8), so every XCD's share is spread over the whole frame and the XCDs run
// out of work together (a contiguous eighth of a frame can cost far more
// than another); each chunk is still a compact run of tiles for the XCD's L2.
// Measured (tools/ab.py): primary 1080p single launch +4.1 %, 4K +4.9 %.
#ifndef VRT_SLICE_CHUNK
#define VRT_SLICE_CHUNK 512       // primary render: 128 tiles x 4 quadrant units
#endif
#ifndef VRT_SEC_SLICE_CHUNK
#define VRT_SEC_SLICE_CHUNK 8192  // config 5: pixels (128 tiles x 64); +2.3 % per frame
#endif
__host__ __device__ inline int slice_size(int units, int x, int ch)
{
        if (ch == 0) {
                int lo, hi;
                queue_range(units, x, lo, hi);
                return hi - lo;
        }
        const int nc = units / ch, rem = units % ch;
        return (nc / 8 + (x < nc % 8 ? 1 : 0)) * ch + (nc % 8 == x ? rem : 0);
}
// the u-th unit of slice x (u < slice_size(units, x, ch))
__host__ __device__ inline int slice_unit(int units, int x, int u, int ch)
{
        if (ch == 0) {
                int lo, hi;
                queue_range(units, x, lo, hi);
                return lo + u;
        }
        return ((u / ch) * 8 + x) * ch + u % ch;
}

// Config-5 ray compaction (k_secondary_p + k_sec_resume).  A
// wave walks one pixel's secondary rays until fewer than `t_first` of them
// are still walking; it then stops, and each of those rays writes its walk
// state -- the ray, the node it was about to visit next and its DFS stack --
// to queue 0.  The resume round (k_sec_stream, or k_sec_resume for films of
// 2^26 pixels or more) continues their walks from the saved states, 64 rays
// to a wave as one pool, to their ends.  The walk after a resume is the walk
// that would have run, so every ray's hit boolean is unchanged.  The pixel's count of hits and of
// rays still out lives in its unused primary-record word (prim[8*pix+7]);
// the ray that brings the outstanding count to zero writes the pixel.
// A queue is cut into chunks of kSpillChunk records: a wave takes a whole
// chunk with one atomic and fills it itself (one atomic per chunk, not per
// stopped pixel, on the queue's counter), and writes the chunk's fill count
// when it moves on; a resume wave takes one chunk at a time.
constexpr int kSpillStack = 10;  // >= the DFS stack (kStack, vrt_kernels.hip)
constexpr uint32_t kSpillChunk = 256;
// 64 B.  The compaction runs only for films under 2^26 pixels and octrees
// under 2^24 nodes (spill_setup), so a pixel and a DFS stack entry each fit a
// word.
struct alignas(16) SpillRec {
        uint32_t pix_smp;  // primary record index (y * W8 + x) | secondary ray index << 26
        uint32_t base;     // the child block the walk was in
        uint32_t mask_sp;  // its children left to visit (8 bits) | stack entries << 8
        float d[3];        // normalised direction (the ray's origin is the pixel's hit point)
        uint32_t stk[kSpillStack];  // DFS stack, bottom first: block << 8 | children left
};
static_assert(sizeof(SpillRec) == 64, "SpillRec layout");
constexpr int kSpillCtrStride = 32;  // one 128-B line per round's counters
constexpr int kSpillMaxRounds = 4;
struct SpillQueues {
        uint32_t *ctr;       // zeroed per frame: [0] chunks taken by phase A, [1] chunks taken by the
                             // stream, [2] records written, [3] chunks the stream left to k_sec_resume,
                             // [4] their pieces taken, [5] stopped rays finished in place (queue full),
                             // [6] pixels deferred to k_secondary_defer, [7] of them taken;
                             // the words of rounds 1..3 ([r * kSpillCtrStride + 2]) stay 0
        uint32_t *dpix;      // the deferred pixels (this rank's pixel indices), one per pixel of the
                             // film at most; NULL: no fast-only kernel
        uint32_t *fill[2];   // [0] records in each chunk of queue 0, written by the chunk's writer;
                             // [1] the chunks the stream left
        SpillRec *rec[2];    // queue 0's records: rec[0] + chunk * kSpillChunk ([1] unused)
        uint32_t nchunks;    // chunks in queue 0; 0 = no compaction
        uint32_t t_first;    // phase-A threshold (walking lanes)
        int32_t stream;      // 1: the resume round streams queue 0 (the only mode)
};

// Tile deal of a multi-rank frame.  The ntx x nty grid of
// 8x8-pixel tiles is cut into G x G blocks of tiles (G = VRT_DEAL_BLOCK);
// the whole blocks are dealt round-robin in block raster order (block j ->
// rank j % nranks), then the tiles outside the whole-block region -- the
// right strip (rows above the bottom strip), then the bottom strip, each in
// raster order -- continue the round robin one tile at a time (leftover i ->
// rank (F + i) % nranks, F = whole blocks).  A rank's tiles are numbered k =
// 0, 1, ...: its blocks' tiles (block order, row-major inside a block), then
// its leftover tiles.  A rank's share is so made of compact G x G regions
// (rays of one region walk the same part of the octree), and every rank gets
// the same number of blocks +-1.  G = 1 is tile t -> rank t % nranks.
//
// Rank 0 lighter (VRT_DEAL_WEIGHT, nranks >= 2): rank 0 also gathers and
// re-assembles the frame, so it is dealt (m-1)/m of another rank's blocks,
// m = max(2, VRT_DEAL_SPAN / nranks) (5/6 at 8 ranks, 11/12 at 4, 23/24 at 2:
// round 5, from every rank's rehearsed step; 7/8 and 15/16 with span 64, and
// no weighting below 4 ranks, left rank 0 the slowest once the collective
// no longer delayed the other ranks).  The whole blocks
// then run in periods of V = m*nranks - 1: position pos = j % V of block j
// goes to rank nranks-1 - pos % nranks (ranks in descending order, rank 0's
// last turn of the period left out); a rank's blocks keep raster order.
#ifndef VRT_DEAL_BLOCK
#define VRT_DEAL_BLOCK 4
#endif
#ifndef VRT_DEAL_WEIGHT
#define VRT_DEAL_WEIGHT 1
#endif
#ifndef VRT_DEAL_SPAN
#define VRT_DEAL_SPAN 48
#endif
struct TileDeal {
        int ntx, nty, nranks, G;
        int bx, by;  // whole blocks per block row / per block column
        int F;       // whole blocks
        int rw;      // width of the right strip (ntx - bx*G)
        int nA;      // tiles of the right strip
        int L;       // leftover tiles (right strip + bottom strip)
        int m, V;    // weighted deal: turns per period of ranks >= 1, period (V = 0: plain round robin)
};
__host__ __device__ inline TileDeal tile_deal(int ntx, int nty, int nranks)
{
        TileDeal d;
        d.ntx = ntx;
        d.nty = nty;
        d.nranks = nranks;
        d.G = nranks > 1 ? VRT_DEAL_BLOCK : 1;  // one rank: raster order
        d.bx = ntx / d.G;
        d.by = nty / d.G;
        d.F = d.bx * d.by;
        d.rw = ntx - d.bx * d.G;
        d.nA = d.by * d.G * d.rw;
        d.L = ntx * nty - d.F * d.G * d.G;
        d.m = VRT_DEAL_WEIGHT && nranks >= 2 ? (VRT_DEAL_SPAN / nranks > 2 ? VRT_DEAL_SPAN / nranks : 2) : 0;
        d.V = d.m ? d.m * nranks - 1 : 0;
        return d;
}
// blocks of rank r in one period of the weighted deal
__host__ __device__ inline int deal_turns(const TileDeal &d, int r)
{
        return r == 0 ? d.m - 1 : d.m;
}
// whole blocks of rank r, and the first leftover index it owns
__host__ __device__ inline int deal_blocks(const TileDeal &d, int r)
{
        if (d.V) {
                const int q = d.nranks - 1 - r, rem = d.F % d.V;
                return (d.F / d.V) * deal_turns(d, r) + (rem > q ? (rem - 1 - q) / d.nranks + 1 : 0);
        }
        return r < d.F ? (d.F - r + d.nranks - 1) / d.nranks : 0;
}
__host__ __device__ inline int deal_l0(const TileDeal &d, int r)
{
        return ((r - d.F) % d.nranks + d.nranks) % d.nranks;
}
// tiles of rank r
__host__ __device__ inline int deal_count(const TileDeal &d, int r)
{
        const int l0 = deal_l0(d, r);
        return deal_blocks(d, r) * d.G * d.G + (l0 < d.L ? (d.L - l0 + d.nranks - 1) / d.nranks : 0);
}
// rank r's k-th tile -> (tx, ty)
__host__ __device__ inline void deal_tile(const TileDeal &d, int r, int k, int &tx, int &ty)
{
        if (d.nranks == 1) {  // raster order (the general form with G = 1, fewer divisions)
                tx = k % d.ntx;
                ty = k / d.ntx;
                return;
        }
        const int G2 = d.G * d.G, nb = deal_blocks(d, r);
        if (k < nb * G2) {
                const int kb = k / G2, w = k % G2;
                int j = r + kb * d.nranks;
                if (d.V) {
                        const int c = deal_turns(d, r);
                        j = (kb / c) * d.V + (d.nranks - 1 - r) + (kb % c) * d.nranks;
                }
                tx = (j % d.bx) * d.G + w % d.G;
                ty = (j / d.bx) * d.G + w / d.G;
                return;
        }
        int li = deal_l0(d, r) + (k - nb * G2) * d.nranks;
        if (li < d.nA) {
                ty = li / d.rw;
                tx = d.bx * d.G + li % d.rw;
        } else {
                li -= d.nA;
                ty = d.by * d.G + li / d.ntx;
                tx = li % d.ntx;
        }
}
// tile (tx, ty) -> its rank r and index k there
__host__ __device__ inline void deal_slot(const TileDeal &d, int tx, int ty, int &r, int &k)
{
        if (tx < d.bx * d.G && ty < d.by * d.G) {
                const int j = (ty / d.G) * d.bx + tx / d.G, w = (ty % d.G) * d.G + tx % d.G;
                if (d.V) {
                        const int pos = j % d.V;
                        r = d.nranks - 1 - pos % d.nranks;
                        k = ((j / d.V) * deal_turns(d, r) + pos / d.nranks) * d.G * d.G + w;
                } else {
                        r = j % d.nranks;
                        k = (j / d.nranks) * d.G * d.G + w;
                }
                return;
        }
        const int li = ty < d.by * d.G ? ty * d.rw + (tx - d.bx * d.G) : d.nA + (ty - d.by * d.G) * d.ntx + tx;
        r = (d.F + li) % d.nranks;
        k = deal_blocks(d, r) * d.G * d.G + li / d.nranks;
}

// Camera + film constants for ray generation (T1), computed on the host.
struct CamParams {
        float s[3], u[3], nf[3], e[3];  // columns of C_
        float origin[3];                // point_transform(C_, {})
        float z;                        // -(film.h / (2*tanf(fov/2)))
        float tmin, tmax;               // near, far
        int32_t nx, ny;
};

// Per-sample outputs (device pointers, any may be null).
struct SampleOut {
        int32_t *hit;
        int32_t *tri;
        uint32_t *vox;
        float *rgb;
        uint32_t *cnt;
};

struct RenderParams {
        DevScene sc;
        CamParams cam;
        int32_t ntx, nty;      // 8x8 tiles in the render area
        int32_t rank, nranks;  // this rank's tiles: tile_deal / deal_tile
        int32_t tiles_this_rank;
        int32_t image_layout;  // 1: out is nx*ny*3 image; 0: packed tiles
        int32_t test_flags;    // vrt_set_test_flags (VRT_TEST_FORCE_DEFER)
        int32_t ty0;           // primary render: first tile row of the band rendered (the tile grid
                               // is rows [ty0, ty0 + nty) of the film; 0 = the whole film)
        float *out;
        SampleOut so;
        WorkQueue q;           // persistent launches only
        // nranks > 1: this rank's tiles in deal order, tx | ty << 16 each
        // (k_deal_map, cached per scene), read with a scalar load instead of
        // tile_deal / deal_tile's divisions per unit; nullptr: computed
        const uint32_t *tile_xy;
        // one rank: ceil(2^40 / ntx), so a tile index k < 2^24 splits into
        // (k % ntx, k / ntx) with one multiply (rank_tile); 0: divide
        uint64_t ntx_magic;
};

// ---- full trace() -------------------------------------
// Per-node cone-tracing state (80 B): VoxelOctree::coverage and illum[6]
// (VRT/voxel_octree.h:64-70), indexed like NodeRec.
struct alignas(16) LMRec {
        float cov;
        float illum[18];
        float pad;
};
static_assert(sizeof(LMRec) == 80, "LMRec must be 80 B");

// Light pass (VRT/main.cc:79-97) over r's film: every sample of the
// canonical single-threaded order k (render_mt task t = tx*8+ty of
// ptx x pty pixels, row-major, samples 0..3) that hits takes the next slot
// j of a compact list (one atomic add per wave) and writes keys[j] = hit leaf
// << kbits | k, vals[j] = j and samp[6j..6j+5] = get_diffuse rgb, isect
// normal; *count ends as the number of hits.  Sorting the pairs by key puts
// each leaf's samples together in canonical order.
struct LightParams {
        RenderParams r;
        int32_t ptx, pty;
        int32_t kbits;       // bits of the canonical index k
        unsigned int *count;
        uint64_t *keys;
        uint32_t *vals;
        float *samp;
        unsigned int *tail_n;  // deferred samples (k_light_tail): count, then work unit << 6 | lane
        uint32_t *tail;
};

// Several lights into one light map (vrt_lightmap_build_lights): one march
// over the concatenated work units of this rank's share of every light film.
// Light l owns the global units [unit_begin, unit_end[l]); its samples'
// canonical indices follow those of lights 0..l-1 (key_base = their whole
// films' sample count), so the sorted lists sum a leaf's samples light after
// light, as the reference's light block run once per light does.  The whole
// table is a kernel argument (under the 4 KB limit, checked below): a
// block's light is block-uniform, so its entry comes by scalar loads.
struct LightEntry {
        CamParams cam;
        int32_t ptx, pty;        // the film's tile grid (= its render_mt task size)
        int32_t unit_begin;
        int32_t pad0;
        const uint32_t *tile_xy; // as RenderParams::tile_xy, for this film's deal
        uint64_t ntx_magic;      // as RenderParams::ntx_magic
        uint64_t key_base;
        float color[3];          // get_diffuse's colour argument
        int32_t pad1;
};
struct LightsParams {
        // the lists, counters, scene, rank and test flags; p.r's camera and
        // tile grid are unused (each light has its own)
        LightParams p;
        int32_t nlights;
        int32_t units;           // unit_end[nlights - 1]
        // prefix sums of the lights' units; INT32_MAX from nlights on
        int32_t unit_end[VRT_MAX_LIGHTS];
        LightEntry e[VRT_MAX_LIGHTS];
};
static_assert(sizeof(LightsParams) <= 4096, "LightsParams must fit the kernel-argument limit");

// Cone-tracing render (trace(), VRT/main.cc:10-30 + cone_trace,
// VRT/voxel_octree.cc:276-330).  split_up[e]: smallest float x in
// [2^e, 2^(e+1)) with (int)log2f(x) == e+1 under the host libm (the same
// log2f the oracle and the reference's float path call), +inf if none.
struct TraceParams {
        RenderParams r;
        const LMRec *lm;
        const float4 *cc;          // per node: box centre xyz, word a (cone descent)
        const uint32_t *lm_bad;    // != 0: some illum is not finite (exact slow path)
        const float4 *cells;       // per node: the cell (lo.xyz, hi.xyz) of the descent to it
        float mindist, maxdist;
        float split_up[64];
        // split_bound[k] (k = 1..63) = the largest cone diameter whose split
        // level (int)log2f(maxdist / diam) -- split_level_of(fl(maxdist /
        // diam)) -- is >= k (0 if none): the level is non-increasing in diam,
        // so it is the count of bounds >= diam, kept by a cursor as a cone's
        // diameter grows instead of a division per step
        float split_bound[64];
        // split path (rec != nullptr): per-sample records of the primary
        // pass (4 x float4: hit point | hit flag, normal, albedo or sky,
        // the hit leaf and -d), tiles_this_rank*256 slots, read by k_cones_film
        float4 *rec;
        // the primary pass's deferred samples (k_trace_prim_tail): count, slots
        unsigned int *tail_n;
        uint32_t *tail;
        // the cone march's step table (kConeSteps entries) and its length,
        // written by k_cone_steps (launched after k_trace_prim)
        float4 *steps;
        int *nsteps;
        int32_t build_steps;  // launch_trace_prim rebuilds the table (k_cone_steps)
};
// Capacity of TraceParams::steps.  A cone's distance grows by >= 11.5 % a
// step (diam >= 2 * aperture * dist), so even maxdist / mindist = 2^128
// takes < 820 steps; a longer sequence (not reachable for finite scenes)
// is flagged (-1) and the march computes its steps inline.
constexpr int kConeSteps = 1024;

// One launch of the batched trace() / cone_trace (vrt_trace_batch,
// vrt_cone_trace_batch): device pointers, n elements.  rays = vrt_ray (8
// floats each) or isects = vrt_isect (6 floats each); hits = vrt_hit records
// (9 words each); hits and the three float parts may be null.
struct BatchIO {
        const float *rays;
        const float *isects;
        int64_t n;
        float *rgb;
        uint32_t *hits;
        float *indirect, *direct, *albedo;
};

// One launch of the light-probe gather (vrt_probe_gather): n probes
// {o xyz, r} and their outputs in device memory; `points` are the host's
// npoints sample points (launch_probe_gather puts them on the device through
// kernel arguments, behind the trace records: TraceParams::tail).
constexpr int kProbeSGs = 14;
constexpr int kProbeMaxPoints = 1024;
struct ProbeIO {
        const float *probes;  // n x 4
        int64_t n;
        int32_t npoints;
        float res;            // the ray's tmin = r + res
        float light[3];
        float *sgs;           // 14 n vrt_sg (7 floats each)
        float *terms;         // 3 * 14 * npoints * n floats, or null
        const float *points;  // device: npoints x 3 (set by the launcher)
};

// Probe membership of a scene built with light probes as voxels
// (vrt_scene_create_probes): side arrays beside the octree, so DevScene and
// every triangle-only kernel stay as they are (a leaf's a / b words and the
// content masks count triangles only).  pnode[i]: leaf -> {first entry of its
// probe list in pref, length}; internal node -> {8-bit mask of the children
// with a probe somewhere below, 0}.
struct ProbeDev {
        const uint2 *pnode;     // one per node
        const uint32_t *pref;   // probe indices, leaf lists in probe order
        const float4 *probes;   // {o xyz, r}
        int32_t ntri;           // a probe hit's voxel index is ntri + k
};
// light map of a probe scene: leaves that hold probes but no triangle get
// coverage 1 (cone_trace_init_filter, VRT/voxel_octree.cc:192-199); after
// launch_lm_leaves, before the level filter
hipError_t launch_lm_probe_leaves(const NodeRec *nodes, const uint2 *pnode, int64_t nnodes, LMRec *lm,
                                  hipStream_t st);

// GPU octree build (vrt_build.hip): the host build's
// arrays, produced on `device` and copied back.
struct DeviceBuild {
        std::vector<NodeRec> nodes;        // content masks included
        std::vector<uint32_t> node_vox;
        std::vector<uint64_t> refs;        // sorted (leaf code << 32 | tri)
        std::vector<int64_t> level_begin;  // BFS level ranges (+ end)
        int64_t ninternal = 0;
        double device_ms = 0;              // descent + sorts + flatten + masks
        // with probes (nprobe > 0): the side arrays of vrt_scene, pnode one
        // per node; empty otherwise
        std::vector<uint2> pnode;
        std::vector<uint32_t> pref;
        int64_t probe_leaves = 0;
        bool too_large = false;            // the error is a size limit (VRT_E_INVALID), not the device's
};
// probes / nprobe: the light probes inserted behind the triangles (nprobe
// == 0: a triangle scene, which takes none of the probe launches)
hipError_t build_tree_device(int device, const float *pos, int ntri, const float root_mn[3],
                             const float root_mx[3], int max_depth, const vrt_probe *probes, int nprobe,
                             DeviceBuild *out, std::string *err);

// Host helpers shared by vrt_host.cpp and vrt_multi.cpp (hidden symbols).
// scene_replicate: src's host-side build uploaded to another device.
int scene_replicate(const vrt_scene *src, const vrt_scene_desc *d, int device, vrt_scene **out);
// The trace() frame of one scene in three steps (vrt_host.cpp, "the trace()
// frames"): frame_begin enqueues the light march of rank light_rank of
// light_nranks of the light film's tile deal and, with a view camera, the
// view's primary march on `stream`; frame_wait is the build's one host sync
// and gives the rank's hit lists; frame_finish sorts `total` hits (merged:
// other ranks' lists were appended behind the rank's own), filters, and
// enqueues the cones + film pass.  cam == nullptr: the light map alone.  A
// failed step has released the job; frame_abort releases one that is not
// going on.  frame_check: the arguments alone, nothing enqueued.
struct FrameJob;
struct FrameArgs {
        const char *what;
        bool may_probe;
        const vrt_camera *light_cam;
        const vrt_film *light_film;
        const float *light_color;
        // nlights > 0: the light list of the *_lights calls (k_light_lights),
        // and light_cam / light_film are unused; 0: the one light above
        const vrt_light *lights;
        int nlights;
        int light_rank, light_nranks;
        const vrt_camera *cam;
        const vrt_film *film;
        float min_voxel;
        int rank, nranks, image_layout;
        float *d_out;
        hipStream_t stream;
};
struct LightList {
        uint64_t *keys;  // n keys (leaf << kbits | canonical sample index), room for cap
        float *samp;     // n records of 6 floats, room for 2 * cap
        unsigned int n;
        uint64_t cap;
        hipStream_t stream;  // the scene's stream, where the lists are written and read
};
int frame_check(vrt_scene *s, const FrameArgs &a);
// a light list's own arguments (count, pointers, films, total samples)
int lights_ok(const vrt_light *lights, int nlights);
int frame_begin(vrt_scene *s, const FrameArgs &a, FrameJob **out);
int frame_wait(FrameJob *j, LightList *l);
int frame_finish(FrameJob *j, unsigned int total, bool merged);
void frame_abort(FrameJob *j);
bool scene_has_lightmap(vrt_scene *s);
// the scene's own stream (light pass, filter, probe gather) is idle
int scene_stream_sync(vrt_scene *s);
// the scene belongs to a vrt_multi handle: vrt_scene_update refuses it
void scene_mark_owned(vrt_scene *s);
// memcpy of a large host range over up to 4 threads.
void par_memcpy(void *dst, const void *src, size_t bytes);
// the process-wide vrt_set_test_flags value
int test_flags();
// Owners of the HIP resources the host keeps (device and pinned memory,
// events, streams): move-only, empty when default-constructed, released by
// the destructor.  An empty owner makes no HIP call, so a host-only scene is
// made and destroyed on a machine without a device; none has static storage
// duration (nothing calls into HIP during process teardown).  An owner
// converts to its handle where a HIP call takes one; whoever releases a
// resource that work in flight may still use waits for that work first.
template <class H, hipError_t (*Release)(H)>
class Owner {
public:
        Owner() = default;
        Owner(Owner &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
        Owner &operator=(Owner &&o) noexcept
        {
                if (this != &o) {
                        reset();
                        h_ = o.h_;
                        o.h_ = nullptr;
                }
                return *this;
        }
        ~Owner() { reset(); }
        void reset()
        {
                if (h_)
                        (void)Release(h_);
                h_ = nullptr;
        }
        H get() const { return h_; }
        operator H() const { return h_; }

protected:
        H h_ = nullptr;
};
// alloc() releases what was held; size(): the bytes held
struct DevMem : Owner<void *, hipFree> {
        hipError_t alloc(size_t bytes)
        {
                reset();
                const hipError_t e = hipMalloc(&h_, bytes);
                if (e != hipSuccess)
                        h_ = nullptr;
                n_ = bytes;
                return e;
        }
        template <class T> T *as() const { return static_cast<T *>(h_); }
        size_t size() const { return h_ ? n_ : 0; }

private:
        size_t n_ = 0;
};
struct PinnedMem : Owner<void *, hipHostFree> {
        hipError_t alloc(size_t bytes)
        {
                reset();
                const hipError_t e = hipHostMalloc(&h_, bytes, hipHostMallocDefault);
                if (e != hipSuccess)
                        h_ = nullptr;
                return e;
        }
        template <class T> T *as() const { return static_cast<T *>(h_); }
};
struct Event : Owner<hipEvent_t, hipEventDestroy> {
        hipError_t create(unsigned flags = hipEventDefault)
        {
                reset();
                return hipEventCreateWithFlags(&h_, flags);
        }
};
struct Stream : Owner<hipStream_t, hipStreamDestroy> {
        hipError_t create(unsigned flags = hipStreamNonBlocking)
        {
                reset();
                return hipStreamCreateWithFlags(&h_, flags);
        }
};
// The event of a resource's last user and whether there was one: the next
// user's stream waits for it, the user records it behind its work, the host
// waits for it before the resource goes.  Before the first record() (the
// event may not exist yet) wait() and sync() do nothing and done() is true.
struct LastUse {
        Event ev;
        bool live = false;
        hipError_t create() { return ev.create(hipEventDisableTiming); }
        hipError_t wait(hipStream_t st) const { return live ? hipStreamWaitEvent(st, ev, 0) : hipSuccess; }
        hipError_t record(hipStream_t st)
        {
                const hipError_t e = hipEventRecord(ev, st);
                if (e == hipSuccess)
                        live = true;
                return e;
        }
        hipError_t sync() const { return live ? hipEventSynchronize(ev) : hipSuccess; }
        bool done() const { return !live || hipEventQuery(ev) == hipSuccess; }
};

// A grow-only staging pair kept between calls: cap bytes on the device and
// as many pinned on the host, used on one stream only.
struct Staging {
        DevMem d;
        PinnedMem h;
        size_t cap = 0;
        // room for `bytes`; growing waits for the stream's work on the old pair
        hipError_t grow(size_t bytes, hipStream_t st)
        {
                if (bytes <= cap)
                        return hipSuccess;
                if (hipError_t e = hipStreamSynchronize(st))
                        return e;
                cap = 0;
                d.reset();
                h.reset();
                if (hipError_t e = d.alloc(bytes))
                        return e;
                if (hipError_t e = h.alloc(bytes))
                        return e;
                cap = bytes;
                return hipSuccess;
        }
};

// ---- scene update (vrt_scene_update[_device], vrt_build.hip) ---------------
// Device memory with a capacity: need() keeps what it holds when that
// suffices, so a steady animation allocates nothing per update.
struct GrowMem : DevMem {
        hipError_t need(size_t bytes)
        {
                if (get() && bytes <= size())
                        return hipSuccess;
                return alloc(bytes ? bytes : 16);
        }
};
// The device build's frontier, sort and flatten arrays and the finish
// kernels' scratch.  build_tree_device makes one per call; a scene that is
// updated keeps one (vrt_scene::bscratch), released with the scene.
struct BuildScratch {
        // build_frontier_device: counters, the two frontiers, the level's codes
        // (sorted, unique), hipcub's temporary, the internal codes, the leaf
        // keys (sorted), and the flattened tree
        GrowMem cnt, pa, pb, codes, codes_s, uniq, nuniq, temp, iall, keys, keys_s, inode, nodes, vox, has;
        // ... and the probe frontier with its outputs
        GrowMem qa, qb, pkeys, pkeys_s, pref, pnode, phas;
        // the callers': positions and normals (build_tree_device: the probes in
        // nrm), root-box keys (6 x 8 B) then the box (6 floats) and the bad-probe
        // word, and the finish kernels' ref_tri, per-node lo/hi, chain minima,
        // leaf counts; probes: a probe update's host probes on the device
        GrowMem pos, nrm, root, ref_tri, lohi, chain, counts, probes;

        size_t bytes() const
        {
                size_t b = 0;
                for (const GrowMem *g : { &cnt, &pa, &pb, &codes, &codes_s, &uniq, &nuniq, &temp, &iall, &keys,
                                          &keys_s, &inode, &nodes, &vox, &has, &qa, &qb, &pkeys, &pkeys_s, &pref,
                                          &pnode, &phas, &pos, &nrm, &root, &ref_tri, &lohi, &chain, &counts,
                                          &probes })
                        b += g->size();
                return b;
        }
};
// The frontier build's result, left on the device in the scratch.
struct DeviceTree {
        const NodeRec *nodes = nullptr;
        const uint32_t *node_vox = nullptr;
        const uint64_t *refs = nullptr;    // sorted (leaf code << 32 | tri)
        int64_t nnodes = 0, nrefs = 0, ninternal = 0;
        std::vector<int64_t> level_begin;
        // probe scenes (nprobe > 0)
        const uint2 *pnode = nullptr;
        const uint32_t *pref = nullptr;
        int64_t nprefs = 0;
        const unsigned int *probe_leaves = nullptr;
        bool too_large = false;
};
// The level-synchronous build from device arrays on stream st (d_probes:
// float4 {o, r} per probe or nullptr).  Host reads of the counters wait for
// st.  fail_limit: report the size limit after the frontier has been expanded
// (VRT_TEST_UPDATE_TOO_LARGE).
hipError_t build_frontier_device(BuildScratch &sc, const float *d_pos, int ntri, const float root_mn[3],
                                 const float root_mx[3], int max_depth, const float4 *d_probes, int nprobe,
                                 hipStream_t st, bool fail_limit, DeviceTree *out, std::string *err);
// Root box of ntri triangles as build_tree merges it: NaN ignored, the first
// of equal extremes in (triangle, vertex) order wins.  keys: 6 uint64 of
// device scratch; box: 6 floats on the device (min xyz, max xyz).  With
// nprobe > 0 the probes' faces {o - r, o + r} follow the vertices in probe
// order (3 * ntri + nprobe must not exceed 2^32), and a seventh word behind
// the box receives the lowest index of a probe that vrt_scene_create_probes
// would refuse, 0xFFFFFFFF when there is none.
hipError_t launch_root_box(const float *d_pos, int ntri, const float4 *d_probes, int nprobe, uint64_t *keys,
                           float *box, hipStream_t st);
// counts[0] = leaves, counts[1] = non-empty leaves of nodes[0, n) (zeroed here)
hipError_t launch_leaf_counts(const NodeRec *nodes, int64_t n, unsigned int *counts, hipStream_t st);
// The finish of a build on the device (finish_tree, ref_boxes, march_nodes,
// chain_spacing of vrt_host.cpp restated).  All pointers are device memory.
struct FinishArgs {
        const DeviceTree *tree;
        const float *pos;       // ntri * 9
        const float *nrm;       // ntri * 9 or nullptr (the stored normals stay)
        int ntri;
        int wide;               // RefRec64 records
        int rboxes;             // write the per-record boxes below refs
        int lb_on;              // extent finite and positive: triangle union boxes in xnodes
        double eps;             // ldexp(extent, -16)
        int chain;              // fast_ok: reduce the chain spacing
        void *refs;             // records (boxes below)
        uint32_t *ref_tri;
        XNodeRec *xnodes;
        double *lohi;           // 6 doubles per node (lb_on)
        uint64_t *chain_out;    // 3 ordered keys of the minima, then a "bad" word (chain)
        TriPos *tri_pos;
        TriAttr *tri_attr;
};
hipError_t launch_finish(const FinishArgs &a, hipStream_t st);
// the ordered key of launch_finish's chain minima back to the double
double chain_key_value(uint64_t key);

// A device scene's update in two halves (vrt_host.cpp), so that a vrt_multi
// handle can have every rank refuse before any rank writes.  update_prepare
// is everything that can refuse: it writes only the scene's BuildScratch and
// memory the scene does not read yet, and fills the plan.  update_commit is
// the rest; only a failed launch or copy stops it (VRT_E_DEVICE, the scene's
// contents then undefined).  A plan that is not committed is abandoned by
// destroying it: its grown[] arrays are released and the scene is as it was.
struct UpdatePlan {
        static constexpr int kOwners = 6;  // nodes, node_vox, refs, xnodes, pnode, pref
        double t0 = 0;
        const float *d_pos = nullptr, *d_nrm = nullptr;
        const float4 *d_probes = nullptr;
        bool new_probes = false;
        float root[7] = {};
        DeviceTree tree;
        unsigned int counts[2] = {};
        bool wide = false, fast = false, lb_on = false, rboxes = false;
        float ext = 0.f;
        size_t sz_rbox = 0;
        DevMem grown[kOwners];  // larger arrays made beside the ones in use
};
// pos / nrm / probes as update_device's; fail_limit: VRT_TEST_UPDATE_TOO_LARGE
// for this scene.  The caller holds the scene's mutex over both halves.
int update_prepare(vrt_scene *s, const float *pos, const float *nrm, const vrt_probe *probes, bool on_device,
                   hipStream_t cst, bool fail_limit, UpdatePlan *plan);
int update_commit(vrt_scene *s, UpdatePlan *plan);
// what vrt_scene_update_probes checks of host probes; the scene's argument
// checks for a rank of a handle (where the owned refusal does not apply)
int update_probes_ok(const vrt_probe *probes, size_t n);
int update_multi_args_ok(vrt_scene *s, const float *pos, bool has_probes, const char *what);
// Room in the scene's BuildScratch for positions, and when asked normals and
// probes, arriving from another device: the staging a host array's upload
// would use.  bytes: the three byte counts (0: not asked for).
int update_stage(vrt_scene *s, bool nrm, bool probes, float **d_pos, float **d_nrm, vrt_probe **d_probes,
                 size_t bytes[3]);
// the scene's mutex (vrt_multi_update holds every rank's over both halves)
std::mutex &scene_mutex(vrt_scene *s);
// what a replica must share beyond its arrays: record format, chain spacing
void scene_replica_key(const vrt_scene *s, int *wide, float wmin[3]);
int scene_device(const vrt_scene *s);
size_t scene_nprobe(const vrt_scene *s);
// VRT_TEST_MULTI_DIVERGE: flip the lowest bit of the first float of TriAttr
int scene_test_flip_attr(vrt_scene *s);

// The digest of vrt.h (vrt_build.hip).  One launch for all items (blockIdx.y):
// out[i] += digest of item i; out is zeroed on st first.
constexpr int kDigestItems = 10;
struct DigestItems {
        const void *p[kDigestItems];
        int64_t bytes[kDigestItems];  // multiples of 4; 0 = absent
        int n;
};
hipError_t launch_digest(const DigestItems &it, uint64_t *out, hipStream_t st);
int64_t digest_pass_words();

// Kernel launchers (vrt_kernels.hip)
// Which primary-render kernel launch_render runs: the one-wave grid
// (k_render: instrumented, per-sample outputs, large-leaf scenes), the
// persistent kernel (k_render_p<false>) or the persistent fast-only kernel
// + its deferred-unit pass (k_render_p<true> + k_render_defer).  The
// persistent kinds take their units from p.q.
enum RenderKind { kRenderGrid = 0, kRenderPersist = 1, kRenderPersistFast = 2 };
RenderKind render_kind(const RenderParams &p, bool instrumented);
// upper bound on the camera rays of the film that fail the fast-only
// kernel's per-wave check (vrt_kernels.hip; cached for the last 32 cameras)
int64_t camera_defer_bound(const CamParams &c);
// *q_waves = the failing adds each slice counter receives (the waves
// launched that visit it), slice_units[x] = the units of slice x (all 0 when
// no work queue was used), for the queue bases
// ord_wmin: the scene's child-centre spacings of the chain order (3 floats,
// vrt_scene::ord_wmin; nullptr or zeros = sort every expansion)
// entry: the launch's beam-entry records (kEntryWords words per unit of the
// rank's share; the persistent fast-only kind fills and reads them), or
// nullptr
hipError_t launch_render(const RenderParams &p, bool instrumented,
                         hipStream_t st, int *q_waves, int slice_units[8], const float *ord_wmin = nullptr,
                         uint32_t *entry = nullptr);
// resident blocks of the persistent render / secondary kernels on the
// current device
hipError_t persistent_blocks(int *render_blocks, int *sec_blocks);
bool secondary_uses_queue(const DevScene &sc);
// pd != nullptr (a probe scene, even_invisible): the mixed march, which takes
// no chain order
hipError_t launch_ray_march(const DevScene &sc, const void *d_rays, int64_t n, void *d_hits, hipStream_t st,
                            const float *ord_wmin = nullptr, const ProbeDev *pd = nullptr);
hipError_t launch_unpack(int nx, int ny, int ntx, int nty, int nranks,
                         int tiles_per_rank, const float *src, float *dst,
                         hipStream_t st);
hipError_t launch_pack_c(int nx, int ny, int rank, int nranks, int comps, const float *img, float *dst,
                         hipStream_t st);
hipError_t launch_unpack_c(int nx, int ny, int nranks, int tiles_per_rank, int comps, const float *src, float *dst,
                           hipStream_t st);
// A side stream of a compaction set and its fork / join events: the
// deferred pixels' exact walk (k_secondary_defer) runs there beside the
// streaming resume instead of after it on the launch's stream.
struct SideLaunch {
        hipStream_t st;
        hipEvent_t fork, join;
};
// The share-sized primary pass of a config-5 launch (k_primary1_share: only
// the records of the rank's own tiles are written) instead of the whole-film
// one.  hits: nullptr, or a zeroed device counter that receives the number of
// the rank's pixels whose primary ray hit.
struct PrimShare {
        unsigned long long *hits;
};
// q: the launch's work queue (persistent kernel) or nullptr (one wave per
// pixel); side: nullptr = every kernel on st; share: nullptr = the whole-film
// primary pass
hipError_t launch_secondary(const RenderParams &rp, int spp, int rank,
                            int nranks, float res, float *prim, float *vis,
                            int32_t *s_hit, int32_t *s_tri, uint32_t *s_vox,
                            const WorkQueue *q, hipStream_t st, int *q_waves, int slice_units[8],
                            const SpillQueues *sq = nullptr, const SideLaunch *side = nullptr,
                            const PrimShare *share = nullptr);
// the compaction settings of this build (VRT_SEC_SPILL*), cap left 0
SpillQueues spill_defaults();
// a path-selecting compile-time switch of the kernel build by name (false:
// unknown name) -- vrt_build_flag
bool build_flag(const char *name, int64_t *value);
hipError_t launch_light(const LightParams &p, hipStream_t st);
hipError_t launch_light_lights(const LightsParams &q, hipStream_t st);
// out[k] = rank's k-th tile of the deal (deal_tile), tx | ty << 16, for k <
// deal_count (ntx, nty < 2^16)
hipError_t launch_deal_map(int ntx, int nty, int nranks, int rank, uint32_t *out, hipStream_t st);
hipError_t light_diag_copy(void *host, size_t bytes);  // VRT_LIGHT_DIAG builds
// samp: n x 6 floats followed by room for their sorted copy (n x 6);
// seg_start: max_seg entries (>= non-empty leaves), nseg zeroed (by
// launch_lm_leaves); seg_end: one entry per node (each hit leaf's run end is
// written)
// vals[i] = i for i < n: the slots of a hit list merged from several ranks'
hipError_t launch_lm_slots(uint32_t *vals, int64_t n, hipStream_t st);
hipError_t launch_lm_accum(int64_t n, const uint64_t *keys_sorted, const uint32_t *vals_sorted, int kbits,
                           const float *samp, uint32_t *seg_start, unsigned int *nseg,
                           int64_t max_seg, uint32_t *seg_end, LMRec *lm, hipStream_t st);
// every leaf's coverage and (zero) illum; also zeroes the light map's
// counters (the finiteness flag, the hit, deferred-sample and run counts) --
// the first kernel of a light-map build, so nothing is cleared by a memset
hipError_t launch_lm_leaves(const NodeRec *nodes, int64_t nnodes, LMRec *lm, uint32_t *bad, unsigned int *count,
                            unsigned int *tail_n, unsigned int *nseg, hipStream_t st);
hipError_t launch_lm_level(const NodeRec *nodes, int64_t begin, int64_t end, LMRec *lm, hipStream_t st);
// a frame's two halves.  A probe scene's frame passes pd and sgs: the mixed
// primary pass writes a probe hit's own record and reads neither the SGs nor
// the light map; the cones + film pass colours those records by
// LightProbe::eval over sgs (device, 14 vrt_sg per probe).  fused: the host
// expf's flavour (expf_model), a kernel argument
hipError_t launch_trace_prim(const TraceParams &p, hipStream_t st, const ProbeDev *pd = nullptr);
hipError_t launch_cones(const TraceParams &p, hipStream_t st, const float *sgs = nullptr, int fused = 0);
// the batched trace(): io.n rays in chunks of `chunk` records (p.rec), and
// the batched cone_trace; both build the step table first when p.build_steps
// pd != nullptr (a probe scene): the primary march is the mixed march; a ray
// that ends on a probe is recorded as a zero-coloured miss (rgb and parts +0)
// with its vrt_hit (tri >= ntri) when io.hits is set
hipError_t launch_trace_batch(const TraceParams &p, const BatchIO &io, int64_t chunk, hipStream_t st,
                              const ProbeDev *pd = nullptr);
hipError_t launch_cones_batch(const TraceParams &p, const BatchIO &io, hipStream_t st);
// the light-probe gather: io.n probes in chunks of `chunk` probes (p.rec
// holds 14 * npoints records per probe of a chunk, p.tail the points);
// host_points = npoints x 3 floats on the host
hipError_t launch_probe_gather(const TraceParams &p, const ProbeIO &io, const float *host_points, int64_t chunk,
                               hipStream_t st);
// out[k] = expf_model(bits first + k * stride), k < n (k_selftest_expf)
hipError_t launch_selftest_expf(uint32_t first, uint32_t stride, int64_t n, int fused, float *out, hipStream_t st);
// y[i] = expf_model(x[i]) on the device (device arrays)
hipError_t launch_expf_model(const float *x, int64_t n, int fused, float *y, hipStream_t st);
// vrt_probe_eval / vrt_probe_shade_hits over device arrays
hipError_t launch_probe_eval(const float *sgs, int64_t n, const float *dirs, int64_t m, int fused, float *rgb,
                             hipStream_t st);
hipError_t launch_probe_shade_hits(const void *hits, int64_t n, const ProbeDev &pd, int32_t nprobe, const float *sgs,
                                   int fused, float *rgb, float *albedo, hipStream_t st);
// per-node cone-descent records and the light map's finiteness flag
hipError_t launch_lm_aux(const NodeRec *nodes, const LMRec *lm, int64_t n, float4 *cc, uint32_t *bad,
                         hipStream_t st);
// stable radix sort of (key, value) pairs on the low `bits` key bits
// (vrt_build.hip); temp == nullptr queries *temp_bytes
hipError_t sort_pairs_u64(void *temp, size_t *temp_bytes, const uint64_t *keys_in, uint64_t *keys_out,
                          const uint32_t *vals_in, uint32_t *vals_out, int64_t n, int bits, hipStream_t st);
hipError_t launch_rgbe(const float *img, int64_t npx, int comp, uint8_t *out, hipStream_t st);
hipError_t launch_selftest_order(const float *dist, const uint32_t *hm, int64_t n, uint32_t *out,
                                 const float *depth, const int32_t *len, int64_t m, int32_t stride,
                                 int32_t *argmin, hipStream_t st);
// per case: in[21i..] = node box min, max, ray o, d, root box min, max,
// ord_wmin -> out[6i..] (k_selftest_chain)
hipError_t launch_selftest_chain(const float *in, int64_t n, uint32_t *out, hipStream_t st);
hipError_t launch_selftest(const double *mt_in, double *mt_out,
                           const float *sat_in, int32_t *sat_out, int64_t n,
                           hipStream_t st);

}  // namespace vrt
