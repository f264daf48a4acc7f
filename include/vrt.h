/*
 * vrt.h -- C ABI of the MI355X-native voxel-octree ray-march hot path
 * (drop-in for jqly/VoxelRayTrace20190722's per-pixel primary-ray loop).
 *
 * libvrt.so (voxelraytrace20190722_amd/libvrt.so) exports exactly the symbols
 * below.  Conventions: plain pointers and sizes, caller-owned outputs, opaque
 * handles, int status codes (VRT_OK = 0, negative = error; the legacy
 * symbols keep the reference's 1/0 returns), no exceptions or exit() across
 * the ABI.  Reference citations: VRT/x = VoxelRayTrace20190722/x.
 */
#ifndef VRT_H
#define VRT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define VRT_OK 0
#define VRT_E_INVALID (-1)  /* bad argument (NULL, size, depth, id range) */
#define VRT_E_NOMEM (-2)    /* host allocation failed */
#define VRT_E_DEVICE (-3)   /* HIP runtime error (see vrt_last_error) */
#define VRT_E_NODEVICE (-4) /* no usable gfx950 device */
#define VRT_E_IO (-5)       /* file could not be opened / written */

#define VRT_MAX_DEPTH 11    /* voxel ids pack 10 bits per axis */

typedef struct vrt_scene vrt_scene;

/* Triangle soup in obj2voxel's output order (VRT/voxel_octree.cc:305-371);
 * triangle i is gi::Triangle{p0,p1,p2,n0,n1,n2,t0,t1,t2,mtl}
 * (VRT/voxel_octree.h:94-113).  Normals are normalised by the build exactly
 * like Triangle::Triangle (VRT/voxel_octree.cc:426). */
typedef struct {
        int32_t ntri;
        const float *pos;      /* ntri*9 */
        const float *nrm;      /* ntri*9 */
        const float *uv;       /* ntri*6, NULL = all zero (texcoord_index -1) */
        const int32_t *mat;    /* ntri,   NULL = all material 0 */
        int32_t nmat;          /* >= 1 */
        const int32_t *mat_tex;/* nmat texture ids, -1 = untextured (Kd) */
        const float *mat_kd;   /* nmat*3 tinyobj material_t::diffuse */
        int32_t ntex;
        const int32_t *tex_dims;  /* ntex*3 {width, height, channels 1..4} */
        const int64_t *tex_off;   /* ntex byte offsets into tex_data */
        const uint8_t *tex_data;  /* stbi_load(...,0) bytes, row 0 = top */
        int64_t tex_bytes;
} vrt_scene_desc;

/* jql::Ray after construction (VRT/graphics_math.h:1150-1167): d is already
 * normalised; tmin/tmax bound AABB3D::isect (VRT/graphics_math.h:1312). */
typedef struct {
        float o[3];
        float d[3];
        float tmin, tmax;
} vrt_ray;

/* Camera (VRT/camera.h:70-84): C = affine_transform(Mat3{s,up_,-fwd}, eye),
 * column-major.  `origin` = point_transform(C,{}) is cached; the film plane
 * z = -(film.h / (2*tanf(fov/2))) is evaluated on the host per film. */
typedef struct {
        float C[16];
        float fov, near_, far_;
        float origin[3];
} vrt_camera;

/* Film (VRT/camera.h:24-39): physical w,h and pixel counts nx,ny. */
typedef struct {
        float w, h;
        int32_t nx, ny;
} vrt_film;

/* One gi::ray_march result (VRT/voxel_octree.h:87-89). */
typedef struct {
        int32_t hit;      /* 1 = ray_march returned true */
        int32_t tri;      /* index of *voxel_ptr in the input soup, -1 */
        uint32_t voxel;   /* *leaf_ptr's integer coords at max depth:
                             ix | iy<<10 | iz<<20, 0xFFFFFFFF on a miss */
        float hit_p[3];   /* ISect::hit */
        float normal[3];  /* ISect::normal */
} vrt_hit;

typedef struct {
        int64_t nodes, internal, leaves, nonempty_leaves, tri_refs;
        int32_t max_depth, device;
        float root_min[3], root_max[3];
        int64_t device_bytes;
        double build_ms, upload_ms;
        double build_device_ms;  /* GPU part of a VRT_BUILD_DEVICE build (probes included), else 0 */
} vrt_scene_info_t;

/* Optional per-sample outputs of vrt_render (host arrays, index
 * ((py*nx+px)*4 + s), s = gen_rays4 sample order).  Any pointer may be NULL.
 * counters = {A aabb tests, L leaves entered, T triangle tests, H hit} as
 * the reference's ray_march performs them; requesting them
 * selects the instrumented kernel variant. */
typedef struct {
        int32_t *hit;
        int32_t *tri;
        uint32_t *voxel;
        float *rgb;       /* 3 per sample: get_diffuse / sky colour */
        uint32_t *counters;
} vrt_samples;

/* Aggregate counters of one instrumented render (sums over all samples). */
typedef struct {
        uint64_t rays, aabb_tests, leaves, tri_tests, hits;
        double kernel_ms;
} vrt_stats;

/* ---- device / scene ------------------------------------------------- */
int vrt_device_count(int *n);
/* gi::ray_march_init (VRT/voxel_octree.cc:67-75) on the host, then upload
 * of the flattened octree + triangles + textures to `device`.  device < 0
 * builds a host-only scene (info / leaves only; device calls then return
 * VRT_E_NODEVICE). */
int vrt_scene_create(const vrt_scene_desc *desc, int max_depth, int device,
                     vrt_scene **out);
/* Same, with build flags: VRT_BUILD_DEVICE runs the octree build on the GPU
 * (level-synchronous SAT descent + hipCUB sorts + BFS flatten, SURVEY §8
 * f3); the octree is identical to the host build.  Needs device >= 0. */
#define VRT_BUILD_DEVICE 1
/* With VRT_BUILD_DEVICE in vrt_scene_create_probes: the light probes are
 * inserted on the GPU too (see there).  Without probes the bit changes
 * nothing; without VRT_BUILD_DEVICE it is VRT_E_INVALID. */
#define VRT_BUILD_DEVICE_PROBES 4
int vrt_scene_create_ex(const vrt_scene_desc *desc, int max_depth, int device,
                        int flags, vrt_scene **out);
void vrt_scene_destroy(vrt_scene *s);
int vrt_scene_info(const vrt_scene *s, vrt_scene_info_t *info);
/* Bytes per leaf record of the scene's device format: 48 (vertices as
 * floats; the primary walks cull such a leaf's records by per-record boxes)
 * or 64 (scenes with >= 8 records per non-empty leaf on average). */
int vrt_scene_ref_format(const vrt_scene *s, int32_t *record_bytes);
/* Non-empty leaves sorted by voxel id; tris = concatenated leaf lists in
 * insertion (input) order.  Sizes from vrt_scene_info. */
int vrt_scene_leaves(const vrt_scene *s, uint32_t *voxel, uint32_t *count,
                     int32_t *tris);
/* The flattened octree, nodes entries each: box (min xyz,
 * max xyz), word a (first child | 0x80000000 + count for leaves), word b
 * (content mask | first leaf record).  Any output may be NULL. */
int vrt_scene_nodes(const vrt_scene *s, float *box, uint32_t *a, uint32_t *b);

/* ---- camera (host, VRT/camera.cc) ------------------------------------ */
int vrt_camera_init(float fov, const float eye[3], const float spot[3],
                    const float up[3], float near_, float far_,
                    vrt_camera *out);
int vrt_gen_rays4(const vrt_camera *cam, const vrt_film *film, int px, int py,
                  vrt_ray out[4]);
int vrt_gen_rays1(const vrt_camera *cam, const vrt_film *film, int px, int py,
                  vrt_ray out[1]);
/* jql::Ray::Ray(o, d, tmin, tmax): normalises d. */
int vrt_make_ray(const float o[3], const float d[3], float tmin, float tmax,
                 vrt_ray *out);
/* AABB3D::isect(ray, nullptr) on the host (box = min xyz, max xyz). */
int vrt_aabb_isect(const float box[6], const vrt_ray *ray);
/* *bound = an upper bound on the gen_rays4 rays of the film with a direction
 * component |d_q| < 2^-64 (an exact zero included): the rays the fast-only
 * persistent render defers to its exact pass.  0 certifies that the frame
 * needs no deferred pass (it is then not launched); INT64_MAX when a camera
 * term is not finite.  Never below the true count. */
int vrt_camera_defer_bound(const vrt_camera *cam, const vrt_film *film, int64_t *bound);

/* ---- the hot path ------------------------------------------------------ */
/* Primary render = the per-pixel loop of VRT/main.cc:118-123 with the
 * primary shading contract (hit: Triangle::get_diffuse(isect, ray, (1,1,1));
 * miss: sky lerp, VRT/main.cc:18-20), 4 gen_rays4 samples accumulated with
 * Film::add(c * .25f).  Pixels outside render_mt's 8x8 tile grid
 * (px >= 8*(nx/8) or py >= 8*(ny/8), VRT/camera.h:45-61) stay 0.
 * Film index is y*nx+x (the reference's y*ny+x, VRT/camera.cc:19, agrees for
 * square films).  rgb: host nx*ny*3 floats.  samples / stats may be NULL. */
int vrt_render(vrt_scene *s, const vrt_camera *cam, const vrt_film *film,
               float *rgb, const vrt_samples *samples, vrt_stats *stats);

/* Device-resident variant (inputs/outputs in HBM, enqueued on `stream`, a
 * hipStream_t or NULL for the null stream; no host synchronisation).
 * Screen = the ntx x nty grid of 8x8-pixel tiles (ntx = nx/8, nty = ny/8).
 * The tile deal (one rule for every multi-rank entry point): with
 * G = vrt_tile_deal_block() (G = 1 when nranks == 1), the whole G x G blocks
 * of tiles are dealt round-robin in block raster order (block j -> rank
 * j % nranks; from 2 ranks on rank 0, which also gathers and re-assembles,
 * is dealt (m-1)/m of a share, m = max(2, 48/nranks): block j -> rank
 * nranks-1 - (j % V) % nranks with V = m*nranks - 1, a rank's blocks in
 * raster order); the tiles outside the whole-block region -- the right strip
 * (rows ty < G*(nty/G), columns tx >= G*(ntx/G)), then the bottom strip, each
 * in raster order -- continue the deal one tile at a time (leftover i ->
 * rank (F + i) % nranks, F = number of whole blocks).  A rank's k-th tile:
 * its blocks' tiles first (block order, row-major inside a block), then its
 * leftover tiles.  This call renders this rank's tiles into d_out packed
 * tile-major: d_out[(k*64 + (y%8)*8 + x%8)*3 + c], sized
 * vrt_tiles_per_rank()*192 floats (the largest share).  rank=0, nranks=1
 * with image_layout=1 writes the nx*ny*3 image directly instead. */
int vrt_tiles_per_rank(const vrt_film *film, int nranks);
/* Launch hint: the caller keeps `n` frames in flight on different streams
 * (n >= 2) or renders one at a time (n = 1, the default).  With n >= 2 a
 * persistent render grid takes half of the resident workgroup slots, so
 * consecutive frames share the chip and one frame's latency-bound ramp-down
 * runs beside the next frame; results are identical either way.  Applies to
 * the device entry points (vrt_render_tiles_device); the synchronous
 * vrt_render always uses the whole chip. */
int vrt_scene_set_frames_in_flight(vrt_scene *s, int n);
int vrt_tile_deal_block(void);
/* The deal as tables (host, no device): for every tile ty*ntx+tx, its rank
 * and its index k in that rank's buffer. */
int vrt_tile_deal_map(const vrt_film *film, int nranks, int32_t *rank_of_tile, int32_t *slot_of_tile);
int vrt_render_tiles_device(vrt_scene *s, const vrt_camera *cam,
                            const vrt_film *film, int rank, int nranks,
                            int image_layout, float *d_out, void *stream);
/* Rank 0 after the gather: d_gathered = nranks * tiles_per_rank * 192 floats
 * (rank-major) -> d_image nx*ny*3 (pixels outside the tile grid zeroed). */
int vrt_unpack_tiles_device(const vrt_film *film, int nranks,
                            const float *d_gathered, float *d_image,
                            void *stream);
/* The same deal for images of `comps` floats per pixel (config 5's
 * visibility image: comps = 1).  Pack: rank `rank`'s tiles of d_image
 * (ny, nx, comps) -> d_packed, tile k at k * 64 * comps, pixels row-major in
 * the tile (tiles_per_rank * 64 * comps floats hold any rank's share).
 * Unpack (rank 0 after the gather): d_gathered = nranks * tiles_per_rank *
 * 64 * comps floats, rank-major -> d_image (zero outside the tile grid). */
int vrt_pack_tiles_c_device(const vrt_film *film, int rank, int nranks, int comps, const float *d_image,
                            float *d_packed, void *stream);
int vrt_unpack_tiles_c_device(const vrt_film *film, int nranks, int comps, const float *d_gathered, float *d_image,
                              void *stream);
/* Device time of the last render kernel enqueued by this thread on `s`
 * (HIP events around the launch, on its stream). */
int vrt_last_kernel_ms(vrt_scene *s, float *ms);

/* SURVEY §8(d) config 5 (stochastic secondary rays, divergent traversal):
 * per pixel of the 8*(n/8) render area a pixel-centre primary ray
 * (gen_rays1); on a hit, jql::PCG seeded 0xc01dbeef ^ (py*nx+px) draws `spp`
 * (1..64) points with jql::random_point_in_unit_sphere (libstdc++'s
 * uniform_real_distribution<float>{-1,1} mapping) and each traces
 * Ray{isect.hit, isect.normal + p, res, FLT_MAX} (VRT/voxel_octree.cc:
 * 600-603 pattern; res = min(root.size()/2^max_depth), VRT/main.cc:69-70).
 * vis[py*nx+px] = misses/spp (1 on a primary miss, 0 outside the area).
 * Per-ray ids (index (py*nx+px)*spp + s) may be NULL; *rays (may be NULL)
 * = rays traced (primary + secondary). */
int vrt_render_secondary(vrt_scene *s, const vrt_camera *cam,
                         const vrt_film *film, int spp, float *vis,
                         int32_t *s_hit, int32_t *s_tri, uint32_t *s_vox,
                         int64_t *rays);
/* Device-resident variant: rank `rank` of `nranks` writes its pixels (its
 * 8x8-pixel tiles of the tile deal, vrt_render_tiles_device) into d_vis (nx*ny floats, caller-zeroed:
 * a sum-reduce over ranks assembles the image exactly); d_prim = scratch of
 * 8*(nx/8)*8*(ny/8)*8 floats. */
int vrt_render_secondary_device(vrt_scene *s, const vrt_camera *cam,
                                const vrt_film *film, int spp, int rank,
                                int nranks, float *d_prim, float *d_vis,
                                void *stream);
/* One rank's config-5 share, packed for the gather: the share-sized primary
 * pass over this rank's tiles of the deal, the secondary walk of
 * vrt_render_secondary_device, then this rank's tiles of d_vis packed
 * tile-major into d_packed (vrt_pack_tiles_c_device with comps = 1:
 * tiles_per_rank * 64 floats).  d_prim: scratch, 8*(nx/8)*8*(ny/8)*8 floats;
 * records of tiles not dealt to this rank are neither written nor read.
 * d_vis: scratch, nx*ny floats, need not be zeroed; only this rank's pixels
 * are written.  d_prim_hits (may be NULL): set to the number of this rank's
 * pixels whose primary ray hit.  nranks == 1 is allowed (raster deal).
 * Enqueued on `stream`, no host synchronisation. */
int vrt_render_secondary_tiles_device(vrt_scene *s, const vrt_camera *cam, const vrt_film *film, int spp,
                                      int rank, int nranks, float *d_prim, float *d_vis, float *d_packed,
                                      uint64_t *d_prim_hits, void *stream);

/* Batched gi::ray_march (VRT/voxel_octree.cc:131-188) on host arrays. */
int vrt_ray_march_batch(vrt_scene *s, const vrt_ray *rays, int64_t n,
                        vrt_hit *hits);
/* Device-resident variant (d_rays / d_hits in HBM). */
int vrt_ray_march_batch_device(vrt_scene *s, const vrt_ray *d_rays, int64_t n,
                               vrt_hit *d_hits, void *stream);

/* Device copies of the fp64 Moller-Trumbore and fp32 SAT leaves (the exact
 * code the kernels inline), run on n host-array cases for parity tests.
 * mt_in: n*15 doubles {orig,dir,v0,v1,v2}; mt_out: n*4 doubles
 * {ret, t, u, v} (t,u,v = 0 unless ret == 1).  sat_in: n*15 floats
 * {center, half, tri[9]}; sat_out: n ints. */
int vrt_device_selftest(int device, const double *mt_in, double *mt_out,
                        const float *sat_in, int32_t *sat_out, int64_t n);

/* Test hook: process-wide flags read by every later render launch.
 * VRT_TEST_FORCE_DEFER makes the persistent fast-path kernel defer every
 * unit to its exact fallback pass (k_render_defer), so tests can pin that
 * rarely taken path against the oracle.  0 = normal operation. */
#define VRT_TEST_FORCE_DEFER 1
/* VRT_TEST_FAIL_LAUNCH makes every fast-path render launch report a launch
 * failure after its first kernel is enqueued (the error path that must
 * leave the scene's work-queue slot usable by later launches). */
#define VRT_TEST_FAIL_LAUNCH 2
/* VRT_TEST_SPILL_ALL makes config-5's ray compaction stop a wave's rays as
 * soon as one of them has ended (every resume round but the last likewise),
 * so that nearly every secondary ray is saved and resumed at least once. */
#define VRT_TEST_SPILL_ALL 4
/* VRT_TEST_VIRTUAL_RANKS_N(n) (2 <= n <= 16), read by vrt_scene_create_multi:
 * a one-device mask creates n *virtual* ranks on that device -- n scene
 * replicas, n streams, the same per-rank send buffers, gather buffer, tile
 * deal and unpack as n devices -- with the RCCL gather replaced by
 * device-to-device copies of each rank's buffer into its slot of rank 0's
 * receive buffer (ordered like the collective: after the rank's render on
 * its stream, before rank 0's unpack).  RCCL refuses duplicate devices; this
 * runs the n-rank frame on a one-GPU box.  Handles created without it are
 * unaffected. */
#define VRT_TEST_VIRTUAL_RANKS 8
/* VRT_TEST_STREAM_LEFTOVER makes config-5's streaming resume round leave
 * every odd chunk of saved rays to its batch-pool launch (the path a chunk
 * with a degenerate ray takes). */
#define VRT_TEST_STREAM_LEFTOVER 16
/* VRT_TEST_LIGHT_TAIL makes the light pass hand every sample to its tail
 * launch (8 lanes per sample; the path of samples whose walk passes the
 * light pass's triangle-test budget). */
#define VRT_TEST_LIGHT_TAIL 32
/* VRT_TEST_PRIM_TAIL does the same for the primary pass of the cone-traced
 * render (vrt_render_trace*, vrt_trace_frame_device). */
#define VRT_TEST_PRIM_TAIL 64
/* VRT_TEST_SEC_DEFER: config 5's fast-only walk kernel defers every odd
 * pixel of its rank to the exact-walk launch after it (k_secondary_defer),
 * as it does a pixel with a ray off the fast walk. */
#define VRT_TEST_SEC_DEFER 128
#define VRT_TEST_VIRTUAL_RANKS_N(n) (VRT_TEST_VIRTUAL_RANKS | ((n) << 8))
/* VRT_TEST_SMALL_BATCH_CHUNK (the next free bit: bits 8..15 hold the virtual
 * rank count) makes vrt_trace_batch[_device] work in chunks of 200 rays, so
 * the chunk seams are reached by small batches. */
#define VRT_TEST_SMALL_BATCH_CHUNK 0x10000
/* VRT_TEST_SMALL_PROBE_CHUNK (the bit after it, unused before) makes
 * vrt_probe_gather[_device] work in chunks of 2 probes. */
#define VRT_TEST_SMALL_PROBE_CHUNK 0x20000
/* VRT_TEST_SMALL_BEAM_ENTRY: the persistent primary render takes the beam
 * entry for a one-rank frame of any size; without it only
 * frames of at least 32,640 units (4x4-pixel quadrants) do, because the
 * pre-pass costs a small frame more than it saves. */
#define VRT_TEST_SMALL_BEAM_ENTRY 0x40000
/* VRT_TEST_UPDATE_TOO_LARGE makes the device build of vrt_scene_update[_device]
 * and vrt_scene_update_probes[_device]
 * report its size limit ("octree too large") after the frontier has been
 * expanded: the refusal a huge scene would meet, which must leave the scene
 * on its previous geometry.  A host-side error return. */
#define VRT_TEST_UPDATE_TOO_LARGE 0x80000
/* VRT_TEST_MULTI_REFUSE_LAST: in vrt_multi_update[_device] the last rank's
 * prepare reports the build's size limit (as VRT_TEST_UPDATE_TOO_LARGE does,
 * for that rank only) while the other ranks succeed: the refusal of one rank
 * must leave every rank on its previous geometry. */
#define VRT_TEST_MULTI_REFUSE_LAST 0x100000
/* VRT_TEST_MULTI_DIVERGE: after a successful commit of vrt_multi_update
 * [_device] the lowest mantissa bit of the first float of the last rank's
 * TriAttr array is flipped (a 4-byte device copy of a normal component), so
 * that VRT_MULTI_UPDATE_VERIFY has a real one-bit difference to report. */
#define VRT_TEST_MULTI_DIVERGE 0x200000
int vrt_set_test_flags(int flags);
/* The current vrt_set_test_flags value (so a caller can restore it). */
int vrt_test_flags(void);

/* Diagnostic: the beam-entry records of the scene's last persistent primary
 * render (builds with VRT_BEAM_ENTRY), one per 4x4-pixel unit
 * of the rank's share in unit order (4 * tile + quadrant), 16 words each:
 * word 0 = 0xFFFFFFFF ("no entry"), else the number of stack entries | 0x100
 * when the unit's rays take the chain order; words 2 + 2i, 3 + 2i = entry i
 * (first child's node index, order | count << 24).  Waits for that launch;
 * *units = its unit count (0: there was none), at most max_units records are
 * copied to out. */
int vrt_debug_beam_entries(vrt_scene *s, uint32_t *out, int64_t max_units, int64_t *units);

/* Diagnostic: the records appended to each compaction queue (phase A, then
 * resume rounds 1..3; with the one streaming resume round only queue 0 is
 * used) by the scene's last config-5 launch; waits for it.  All 0 when that
 * launch used no compaction. */
int vrt_secondary_spill_counts(vrt_scene *s, int64_t counts[4]);
/* Diagnostic: the scene's last config-5 launch's compaction, waits for it:
 * stats[0] records queued, [1] stopped rays finished in place because the
 * queue was full, [2] queue chunks taken, [3] chunks allocated, [4] chunks
 * left to the batch-pool launch after the streaming round, [5] bytes per
 * record, [6] pixels deferred from the fast-only walk kernel to the exact
 * walk (a ray with a zero or tiny direction component).  All 0 when that
 * launch used no compaction. */
int vrt_secondary_spill_stats(vrt_scene *s, int64_t stats[7]);
/* Device bytes the scene holds beyond its octree, triangles and textures
 * (vrt_scene_info().device_bytes): per-call scratch kept between calls --
 * config 5's compaction queues (*spill_bytes, may be NULL), the light-map
 * build's scratch and light-map sets, the trace records (the frames' and
 * the batched trace's and the probe gather's one chunk share them), the
 * device staging of the host-array batched trace and probe gather, the host-output image, the tabled tile deals of multi-rank calls (4 B per tile of the
 * rank). */
int vrt_scene_scratch_bytes(vrt_scene *s, int64_t *bytes, int64_t *spill_bytes);

/* The kernels' own travorder sort (std::sort of the 8 Items by dist,
 * VRT/voxel_octree.cc:77-97) and ray_march_isect min_element
 * (VRT/voxel_octree.cc:122-125) on arbitrary inputs, for the pin against
 * the real libstdc++ (tests/golden/travorder_std.cpp).  Per case i:
 * dist[8i..8i+7] and hit_mask[i] (bit ci = child ci's slab test passed) ->
 * orders[6i..6i+5] = {full insertion-sort order (3-bit fields), exact-path
 * hit order | count << 24, rank order | count << 24, two-slot order,
 * 4-slot network order, full-position word} (the last four are the
 * NaN-free fast paths).  Per record list j: depth[j*stride .. +len[j]) ->
 * argmin[j] (the first minimum, -1 when empty). */
int vrt_device_selftest_order(int device, const float *dist,
                              const uint32_t *hit_mask, int64_t n,
                              uint32_t *orders, const float *depth,
                              const int32_t *len, int64_t m, int32_t stride,
                              int32_t *argmin);

/* The walk's chain order (the travorder order of a node's hit children from
 * the ray's octant alone) on arbitrary expansions.  Per case
 * i: cases[21i..21i+20] = node box min, max, ray origin, direction, root box
 * min, max, ord_wmin (the scene constant, vrt_scene_chain_spacing) ->
 * out[6i..6i+5] = {hit mask of the 8 children, sorted order | count << 24,
 * chain order | count << 24, general-form chain order | count << 24, flags
 * (1 the ray passes the criterion, 2 the hit set is a chain, 4 the same by
 * the general form, 8 the ray meets the finite-slab walk's preconditions),
 * the walk's own expansion with its wave votes | count << 24}; order words
 * hold `count` 3-bit fields, first child in bits 0-2. */
int vrt_device_selftest_chain(int device, const float *cases, int64_t n,
                              uint32_t *out);

/* The scene's chain-order constant: per axis the smallest spacing of the two
 * child centres over its internal nodes; zeros = the chain order is off. */
int vrt_scene_chain_spacing(const vrt_scene *s, float out[3]);

/* ---- moving geometry -------------------------------------------------------
 * Replace the scene's vertex positions (ntri*9 floats, the layout of
 * vrt_scene_desc::pos) and, unless nrm is NULL, its vertex normals (ntri*9,
 * normalised as at creation); rebuild octree, leaf records, march records and
 * shading tables.  ntri, uv, materials, textures, max_depth, device unchanged.
 * Afterwards the scene equals, bit for bit, one created with
 * vrt_scene_create_ex(VRT_BUILD_DEVICE) from the same description with these
 * arrays: every query, render and device array; the light map and every other
 * derived state are a fresh scene's (build the light map again), while
 * vrt_scene_set_frames_in_flight, streams, queues and scratch stay.  The call
 * waits for all work the scene has in flight first, on whatever stream it was
 * launched: it synchronises the scene's device.  (Calls on the scene from
 * other threads during an update are the caller's to exclude.)  A device scene
 * rebuilds on the GPU; a host-only scene (device < 0) runs the host build.  A
 * refused update (VRT_E_INVALID: null arguments, a scene with light probes --
 * which vrt_scene_update_probes below moves --, a
 * rank scene of a vrt_multi handle, a size limit of the build; no memory)
 * leaves the scene on its previous geometry, fully usable.  Only VRT_E_DEVICE
 * (a failed launch or copy) can leave it half rebuilt: destroy it then. */
int vrt_scene_update(vrt_scene *s, const float *pos, const float *nrm);
/* The same from device memory on the scene's device.  The arrays are read in
 * `stream` order (NULL = the null stream).  On return the scene is ready and
 * the caller may overwrite the arrays. */
int vrt_scene_update_device(vrt_scene *s, const float *d_pos, const float *d_nrm, void *stream);
/* Wall-clock split of the last update of either kind: {total, GPU (events),
 * copy back, host}. */
int vrt_scene_update_stats(const vrt_scene *s, double ms[4]);
/* The device memory an updated scene keeps for its next update (the build's
 * frontier, sort and flatten arrays and the finish kernels' scratch), which
 * neither vrt_scene_info's device_bytes nor vrt_scene_scratch_bytes counts:
 * *bytes as held on entry; 0 on a scene never updated.  release != 0 frees it
 * (and the spare host mirrors); the next update allocates it again. */
int vrt_scene_update_scratch(vrt_scene *s, int release, int64_t *bytes);
/* Test access: copy one derived device array of the scene to the host.
 * kind: 0 leaf records (48 or 64 B each), 1 per-record boxes (device order, pad excluded),
 * 2 xnodes, 3 TriPos, 4 TriAttr; on a probe scene only (VRT_E_INVALID on any
 * other): 5 pnode (8 B per node), 6 pref (4 B per probe reference), 7 the
 * probes (16 B each).  out == NULL returns only *bytes. */
int vrt_scene_device_array(vrt_scene *s, int kind, void *out, int64_t cap, int64_t *bytes);

/* ---- scene digest ---------------------------------------------------------
 * The digest of a byte array read as W = nbytes / 4 little-endian 32-bit
 * words w_0 .. w_{W-1} (nbytes % 4 != 0: VRT_E_INVALID):
 *   sum over i of mix(((i + 1) * 0x9E3779B97F4A7C15) ^ w_i)   (mod 2^64)
 *   mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
 *           z *= 0x94D049BB133111EB; z ^= z >> 31
 * with i a 64-bit index from the array's first word.  The sum commutes, so
 * every reduction order gives the same word; the empty array digests to 0.
 * vrt_digest_host is the plain statement; vrt_scene_digest runs the device
 * kernel (one launch) over the arrays an update rewrites and waits for it:
 * items 0-7 are vrt_scene_device_array's kinds (an absent array digests to 0),
 * 8 the node records, 9 the nodes' voxel indices.  VRT_E_NODEVICE on a
 * host-only scene.  vrt_device_selftest_digest uploads `bytes` to a 16-byte-
 * aligned buffer + misalign (0, 4, 8 or 12) and runs the kernel's own code;
 * device < 0 is the host model. */
#define VRT_DIGEST_ITEMS 10
int vrt_scene_digest(vrt_scene *s, uint64_t out[VRT_DIGEST_ITEMS]);
int vrt_digest_host(const void *bytes, int64_t nbytes, uint64_t *out);
int vrt_device_selftest_digest(int device, const void *bytes, int64_t nbytes, int misalign, uint64_t *out);

/* ---- multi-device frame (render_mt, VRT/camera.h:42-68,
 * over the GPUs of one node) --------------------------------------------------
 * One handle for the scene replicated on every device of `device_mask` (bit d
 * = HIP device d; rank i = the i-th set bit, rank 0 = the lowest device, which
 * receives and re-assembles the frame) and an RCCL communicator over them
 * (ncclCommInitAll; RCCL is linked into libvrt.so).  The octree is built once
 * on the host (or on the first device with VRT_BUILD_DEVICE) and uploaded to
 * every device.  A frame: rank i renders its tiles of the tile deal
 * (vrt_render_tiles_device with rank i of n) on its device's stream, one
 * ncclGather of the packed tile buffers to rank 0 over xGMI (rank 0's share
 * rendered in place into the receive buffer), then vrt_unpack_tiles_device
 * on rank 0.  Pixels are the single-device render's, bit for bit. */
typedef struct vrt_multi vrt_multi;
int vrt_scene_create_multi(const vrt_scene_desc *desc, int max_depth,
                           uint32_t device_mask, int flags, vrt_multi **out);
void vrt_multi_destroy(vrt_multi *m);
/* devices[i] = rank i's HIP device (n entries, n = set bits of the mask). */
int vrt_multi_devices(const vrt_multi *m, int *n, int32_t *devices);
/* Rank i's scene (borrowed, owned by m): info, single-device entry points. */
int vrt_multi_scene(vrt_multi *m, int rank, vrt_scene **out);
/* The whole frame into a host nx*ny*3 array (index y*nx+x, as vrt_render). */
int vrt_render_multi(vrt_multi *m, const vrt_camera *cam,
                     const vrt_film *film, float *rgb);
/* The whole frame into d_image (nx*ny*3 floats on rank 0's device), ordered
 * after the work already queued on `stream` (a hipStream_t of rank 0's
 * device); work queued on `stream` afterwards sees the image.  stream = NULL:
 * the call returns when the image is complete.  The ranks' renders and the
 * gather run on streams owned by m. */
int vrt_render_multi_device(vrt_multi *m, const vrt_camera *cam,
                            const vrt_film *film, float *d_image,
                            void *stream);
/* The deal of a frame over the devices of a mask (host, no device): per
 * tile ty*ntx+tx, its device and its index in that device's buffer. */
int vrt_multi_tile_map(const vrt_film *film, uint32_t device_mask,
                       int32_t *device_of_tile, int32_t *slot_of_tile);

/* ---- full trace() (VRT/main.cc:10-30, 79-123) -------
 * The reference's actual image: a light pass from a light camera
 * (render_mt + gen_rays4; every hit adds clamp(dot(illum_d[i], n), 0, 1) *
 * get_diffuse to leaf->illum[i]), cone_trace_init_filter, then per camera
 * sample trace(root, ray, 5, true) = sky on a miss, else get_albedo *
 * (6-cone cone_trace + leaf compute_illum(-d)), accumulated with
 * Film::add(c * .25f).  The reference's light-map += races across threads;
 * here the per-leaf sums run in the canonical single-threaded order (task
 * t = tx*8+ty, pixels row-major, samples 0..3), so results are
 * deterministic and bit-identical to the oracle's single-threaded order.
 *
 * vrt_lightmap_build: light pass + filter on the scene's device (blocking);
 * hits (may be NULL) = light samples that hit.  A new build replaces the
 * previous light map. */
int vrt_lightmap_build(vrt_scene *s, const vrt_camera *light_cam,
                       const vrt_film *light_film, int64_t *hits);
/* Per node (vrt_scene_info().nodes entries, BFS order): key = depth << 32 |
 * ix | iy<<10 | iz<<20 (coords at that depth), VoxelOctree::coverage and
 * illum[6][3].  coverage / illum may be NULL. */
int vrt_lightmap_nodes(vrt_scene *s, uint64_t *key, float *coverage,
                       float *illum);
/* Diagnostics of the last light-map build (vrt_lightmap_build[_lights] or a
 * one-call frame): stats = {light samples (64 * (nx/8) * (ny/8) * 4, summed
 * over the lights of a light list), samples that
 * hit, samples whose walk passed the triangle-test budget and was handed to
 * the tail walk}.  All 0 before the first build. */
int vrt_lightmap_stats(vrt_scene *s, int64_t stats[3]);
/* min component of root.size() / powf(2, levels) -- the reference's Res
 * (VRT/main.cc:69-70); levels <= 0 uses the scene's max_depth. */
int vrt_scene_min_voxel(const vrt_scene *s, int levels, float *res);
/* Cone-tracing render with min_voxel_size = min_voxel (<= 0: the scene's
 * Res).  rgb: host nx*ny*3 (index y*nx+x); s_hit / s_rgb optional
 * per-sample outputs ((py*nx+px)*4+s). */
int vrt_render_trace(vrt_scene *s, const vrt_camera *cam, const vrt_film *film,
                     float min_voxel, float *rgb, int32_t *s_hit,
                     float *s_rgb);
/* Device-resident variant with the tile partition of
 * vrt_render_tiles_device. */
int vrt_render_trace_device(vrt_scene *s, const vrt_camera *cam,
                            const vrt_film *film, float min_voxel, int rank,
                            int nranks, int image_layout, float *d_out,
                            void *stream);

/* The whole reference main() frame (VRT/main.cc:75-126) in one call: the
 * light pass + cone_trace_init_filter (as vrt_lightmap_build, on the scene's
 * stream) and, beside them on `stream`, the view's primary march, which reads
 * no light map; the cone-traced shading then waits for the filter.  Values
 * equal vrt_lightmap_build followed by vrt_render_trace_device (same tile
 * deal / layout arguments).  Returns after one host sync (the light pass's
 * hit count, *hits, may be NULL); the image is complete in stream order. */
int vrt_trace_frame_device(vrt_scene *s, const vrt_camera *light_cam,
                           const vrt_film *light_film, const vrt_camera *cam,
                           const vrt_film *film, float min_voxel, int rank,
                           int nranks, int image_layout, float *d_out,
                           void *stream, int64_t *hits);

/* ---- several coloured lights in one light map -----------------------------
 * The reference's light block (VRT/main.cc:80-97) run once per light,
 * lights[0] first, into one map, and one cone_trace_init_filter afterwards.
 * A light is a light camera, its film and the colour the block hands to
 * Triangle::get_diffuse(isect, ray, color) (VRT/voxel_octree.cc:462-469;
 * the reference's driver passes (1,1,1)): a hit sample adds
 * clamp(dot(illum_d[i], normal), 0, 1) * ((albedo * tmp) * color) to
 * leaf->illum[i], componentwise, one rounding per multiplication.  A leaf's
 * sum is one sequential float chain from zero over light 0's samples in the
 * canonical order (vrt_lightmap_build's), then light 1's, and so on: the
 * order of the lights is part of the result's last bits.  One light with
 * colour (1,1,1) gives vrt_lightmap_build's map bit for bit.  Colours are
 * taken as they are (negative, above 1, non-finite).
 *
 * One march, one sort, one sum, one filter and one host sync whatever
 * nlights is.  Each film is checked as vrt_lightmap_build checks its film; a
 * film without a sample (nx < 8 or ny < 8) contributes nothing.
 * VRT_E_INVALID: nlights outside 1..VRT_MAX_LIGHTS, a NULL argument, or more
 * than 2^31 - 1 samples (64 * (nx/8) * (ny/8) * 4 per film) over all lights;
 * nothing is enqueued then and the current light map stays.  The scene's
 * light scratch (vrt_scene_scratch_bytes) holds 72 bytes per sample of the
 * total (keys and slots in and out, the hit records and their sorted copy)
 * plus the sort's own temporary storage.  *hits (may be NULL): the hit
 * samples of all lights.  vrt_lightmap_stats afterwards: the samples marched
 * over all lights, the hits, the samples handed to the tail walk.  A new
 * build replaces the previous light map; every reader of the map works on it
 * unchanged. */
#define VRT_MAX_LIGHTS 16
typedef struct {
        vrt_camera cam;
        vrt_film film;
        float color[3];
} vrt_light;
int vrt_lightmap_build_lights(vrt_scene *s, const vrt_light *lights, int nlights, int64_t *hits);
/* vrt_trace_frame_device / vrt_trace_frame_probes_device with the light list
 * above: values equal vrt_lightmap_build_lights followed by
 * vrt_render_trace_device (on a probe scene: by the probes' gather, then
 * vrt_render_trace_probes_device).  probe_light_color is NOT a light's
 * colour: it is the light_color of vrt_trace_frame_probes_device, the value a
 * probe's gather adds where a gather ray misses (float[3]; NULL keeps the
 * stored SGs; ignored on a scene without probes). */
int vrt_trace_frame_lights_device(vrt_scene *s, const vrt_light *lights, int nlights,
                                  const float *probe_light_color, const vrt_camera *cam,
                                  const vrt_film *film, float min_voxel, int rank, int nranks,
                                  int image_layout, float *d_out, void *stream, int64_t *hits);

/* ---- batched trace() / cone_trace over the caller's rays and points -------
 * The reference's per-ray entry points beside ray_march, as its
 * LightProbe::gather_light uses them: the driver's trace(root, ray, 5, true)
 * (VRT/main.cc:10-30) and gi::cone_trace(root, isect, min_voxel_size)
 * (VRT/voxel_octree.cc:313-330), on the scene's current light map
 * (vrt_lightmap_build / vrt_trace_frame_device; VRT_E_INVALID without one).
 * min_voxel <= 0: the scene's Res.  n == 0 is VRT_OK and touches nothing. */
/* jql::ISect (hit point, normal) as gi::cone_trace takes it */
typedef struct { float hit_p[3]; float normal[3]; } vrt_isect;

/* optional per-ray outputs of vrt_trace_batch; any pointer may be NULL */
typedef struct {
        vrt_hit *hits;     /* n: exactly what vrt_ray_march_batch writes */
        float *indirect;   /* 3n: cone_trace(root, isect, min_voxel) */
        float *direct;     /* 3n: leaf->compute_illum(-ray.d) */
        float *albedo;     /* 3n: get_albedo(isect) */
} vrt_trace_parts;

/* rgb[3i..] = trace(root, rays[i], 5, true): the sky lerp on a miss, else
 * get_albedo * (cone_trace + compute_illum(-d)).  Rays are taken as they are
 * (already constructed, as vrt_ray_march_batch takes them).  On a miss the
 * three float parts are +0 and hits holds the miss record.  Host arrays. */
int vrt_trace_batch(vrt_scene *s, const vrt_ray *rays, int64_t n, float min_voxel,
                    float *rgb /* 3n */, const vrt_trace_parts *parts /* may be NULL */);
/* Device-resident variant: every array in HBM (d_parts is a host struct of
 * device pointers), enqueued on `stream`, no host synchronisation; ordered
 * with frames in flight on other streams through the light-map set's event.
 * Scratch (one chunk of 64-B records) does not grow with n. */
int vrt_trace_batch_device(vrt_scene *s, const vrt_ray *d_rays, int64_t n, float min_voxel,
                           float *d_rgb, const vrt_trace_parts *d_parts, void *stream);
/* rgb[3i..] = gi::cone_trace(root, isects[i], min_voxel) for every element,
 * whatever the point and normal are (there is no notion of a miss). */
int vrt_cone_trace_batch(vrt_scene *s, const vrt_isect *isects, int64_t n, float min_voxel,
                         float *rgb /* 3n */);
int vrt_cone_trace_batch_device(vrt_scene *s, const vrt_isect *d_isects, int64_t n,
                                float min_voxel, float *d_rgb, void *stream);

/* ---- light probes (gi::LightProbe, gi::SG; VRT/voxel_octree.h:120-163,
 * VRT/voxel_octree.cc:497-632) -------------------------------------------
 * LightProbe::gather_light(root, res, light_dir, light_color) for many
 * probes at once, on the scene's current light map: for each of the 14
 * directions dirs_[i] (6 axes, then the 8 cube diagonals) and each sample
 * point r_j the ray Ray{o, r_j + dirs_[i] * 2.6131f, r + res} (tmin = r +
 * res, tmax = FLT_MAX) is marched; a miss adds light_color, a hit
 * cone_trace(root, isect, res); the sum over the points, in point order from
 * zero, divided by (float)npoints is the amplitude of sgs[14 p + i] =
 * SG{litness, dirs_[i], 10}.  light_dir is unused by the reference and is
 * not a parameter.  The marches record no albedo and no direct term. */
#define VRT_PROBE_SGS 14
#define VRT_PROBE_MAX_POINTS 1024
typedef struct { float o[3]; float r; } vrt_probe;
/* gi::SG: amplitude, axis (normalised by the constructor), sharpness */
typedef struct { float a[3]; float d[3]; float s; } vrt_sg;

/* The points LightProbe::LightProbe draws: jql::PCG{seed}, n (1..1024)
 * calls of random_point_in_unit_sphere; pts = 3n floats.  seed 0xc01dbeef,
 * n = 100: the reference's points (every probe has the same ones). */
int vrt_probe_points(uint64_t seed, int n, float *pts);
/* Host arrays.  min_voxel <= 0: the scene's Res.  points == NULL: the
 * reference's 100 points (npoints is ignored); else npoints (1..1024) points
 * of the caller's.  sgs: 14 n records.  terms (may be NULL): 3 * 14 *
 * npoints * n floats, the value each ray added to litness, ray index
 * (p * 14 + i) * npoints + j.  n == 0 is VRT_OK and touches nothing;
 * VRT_E_INVALID without a light map.  Works in chunks of whole probes
 * (about 2^20 rays): the scratch is the batched trace's record block and
 * staging and does not grow with n. */
int vrt_probe_gather(vrt_scene *s, const vrt_probe *probes, int64_t n, float min_voxel,
                     const float light_color[3], const float *points, int npoints, vrt_sg *sgs,
                     float *terms);
/* Device-resident variant: d_probes, d_sgs, d_terms in HBM (points stays a
 * host array: it travels in kernel arguments), enqueued on `stream` with no
 * host synchronisation; ordered with frames in flight and trace batches
 * through the light-map set's event, as vrt_trace_batch_device; reads the
 * light map that is current when it is enqueued. */
int vrt_probe_gather_device(vrt_scene *s, const vrt_probe *d_probes, int64_t n, float min_voxel,
                            const float light_color[3], const float *points, int npoints,
                            vrt_sg *d_sgs, float *d_terms, void *stream);
/* LightProbe::eval on the host: rgb[(p * m + k) * 3 ..] = the sum over probe
 * p's 14 lobes, in order from zero, of SG::eval(dirs[k]) = a * expf(s *
 * (dot(dir, d) - 1)), with the C library's expf (the pinned contract, as the
 * cone step table's log2f).  dirs: 3m floats, used as they are. */
int vrt_probe_eval(const vrt_sg *sgs, int64_t n, const float *dirs, int64_t m, float *rgb);

/* ---- light probes as scene voxels (VRT/main.cc:56-64; LightProbe is a
 * VoxelBase, VRT/voxel_octree.h:120-163) -----------------------------------
 * The driver pushes its probes into the same voxel list as the triangles, so
 * ray_march_init inserts them into the octree, and the view's trace(root,
 * ray, 5, true) marches with even_invisible = true: a probe (is_visible() ==
 * false, VRT/voxel_octree.cc:588-591) can then end a ray.
 *
 * vrt_scene_create_probes: gi::ray_march_init over the triangles followed by
 * the probes (voxel v < ntri = triangle v, voxel ntri + k = probe k).  The
 * root box is AABB{} merged with every triangle box and then with each
 * probe's get_aabb() = {o - r, o + r} (VRT/voxel_octree.cc:541-544), so
 * probes may enlarge it; each probe is inserted after all triangles by
 * insert() (VRT/voxel_octree.cc:41-65) with LightProbe::is_overlap
 * (VRT/voxel_octree.cc:567-586).  A leaf's list is its triangles in input
 * order, then its probes in probe order.  nprobe == 0 or probes == NULL is
 * vrt_scene_create_ex.  Bounds: ntri + nprobe < 2^31, o finite, r finite and
 * >= 0 (r == 0 overlaps nothing).
 *
 * flags: 0 builds on the host.  VRT_BUILD_DEVICE | VRT_BUILD_DEVICE_PROBES
 * (needs device >= 0) runs the whole build on the GPU: the probes are a
 * second frontier of (probe, node) pairs beside the triangles', expanded
 * level by level with LightProbe::is_overlap; a level's internal nodes are
 * those of both frontiers, and the probe lists and masks are written by the
 * device.  Every array equals the host build's, and vrt_scene_info's
 * build_device_ms covers triangles and probes.  VRT_BUILD_DEVICE alone with
 * probes is VRT_E_INVALID (it inserts triangles only), as is
 * VRT_BUILD_DEVICE_PROBES alone or any other bit.  Limits of the device
 * build (VRT_E_INVALID): at every level 8 x the (triangle, node) pairs and
 * 8 x the (probe, node) pairs stay below 2^31 each, and the tree below 2^31
 * nodes.
 *
 * Every visible-only call (vrt_ray_march_batch, vrt_lightmap_build's light
 * pass, vrt_probe_gather, vrt_cone_trace_batch, vrt_render,
 * vrt_render_secondary) runs on such a scene as the reference's ray_march(...,
 * false) does: probes are skipped.  vrt_scene_info's nonempty_leaves and
 * tri_refs keep their triangle meaning; nodes, internal and leaves count the
 * whole tree.  Not available on a probe scene (VRT_E_INVALID; use
 * vrt_trace_batch): vrt_render_trace[_device], vrt_trace_frame_device and
 * vrt_render's instrumented counters.  A probe scene's film frames are
 * vrt_render_trace_probes[_device] and vrt_trace_frame_probes_device below. */
int vrt_scene_create_probes(const vrt_scene_desc *desc, const vrt_probe *probes, int32_t nprobe,
                            int max_depth, int device, int flags, vrt_scene **out);
/* Probes of the scene, leaves that hold at least one probe, and the total
 * length of their probe lists (all 0 for a scene without probes).  Any output
 * may be NULL. */
int vrt_scene_probe_info(const vrt_scene *s, int32_t *nprobe, int64_t *probe_leaves, int64_t *probe_refs);
/* As vrt_scene_leaves: the leaves holding at least one probe sorted by voxel
 * id; probes = concatenated probe indices (0-based) in list order. */
int vrt_scene_probe_leaves(const vrt_scene *s, uint32_t *voxel, uint32_t *count, int32_t *probes);
/* The scene's stored SGs (14 * nprobe records; zero at creation), read by a
 * probe hit's get_albedo. */
int vrt_scene_set_probe_sgs(vrt_scene *s, const vrt_sg *sgs);
int vrt_scene_probe_sgs(const vrt_scene *s, vrt_sg *sgs);
/* VRT/main.cc:104-105: gather_light for every probe of the scene with the
 * reference's 100 points (vrt_probe_gather on the scene's own probes) into
 * the stored SGs.  Needs a light map. */
int vrt_scene_probes_gather(vrt_scene *s, float min_voxel, const float light_color[3]);

/* The update of a probe scene (vrt_scene_create_probes with nprobe >= 1): new
 * positions (required, ntri*9), new normals (NULL: the stored normals stay)
 * and new probe centres and radii (nprobe records; NULL: the probes stay where
 * they are).  ntri, nprobe, uv, materials, textures, max_depth, device
 * unchanged.  Afterwards the scene equals, bit for bit, one created with
 * vrt_scene_create_probes(VRT_BUILD_DEVICE | VRT_BUILD_DEVICE_PROBES) from
 * these arrays -- every query, march, render and device array, the host copy
 * of the probes included -- with the two differences vrt_scene_update
 * documents: derived state is a fresh scene's (no light map:
 * vrt_scene_probes_gather and the trace calls refuse until one is built), and
 * frames in flight, streams, queues, scratch and test flags stay.  The stored
 * SGs (14 per probe) are caller data of unchanged size and stay:
 * vrt_scene_probe_sgs returns the same bytes before and after, whichever copy
 * was the newer one.  Waiting, thread rules and the host-only scene are
 * vrt_scene_update's.  A probe is checked as at creation (centre finite,
 * radius finite and >= 0): a bad one is VRT_E_INVALID with its index.  On a
 * scene without probes: VRT_E_INVALID (use vrt_scene_update).  A refused
 * update (VRT_E_INVALID: null s or pos, a scene without probes, a rank scene
 * of a vrt_multi handle, a bad probe, a size limit of the build -- 3 * ntri +
 * nprobe above 2^32 among them; no memory) leaves the scene on its previous
 * geometry and probes, fully usable; only VRT_E_DEVICE can leave it half
 * rebuilt. */
int vrt_scene_update_probes(vrt_scene *s, const float *pos, const float *nrm, const vrt_probe *probes);
/* The same from device memory on the scene's device; all three arrays are
 * read in `stream` order and are the caller's again on return.  The probes
 * are checked by a kernel, whose flag comes back with the root box: no
 * synchronisation is added for it.  d_probes needs only a float's alignment
 * (a slice of a larger array will do); one that is not 16-byte aligned costs a
 * device-to-device copy of the probes.  A host-only scene: VRT_E_NODEVICE. */
int vrt_scene_update_probes_device(vrt_scene *s, const float *d_pos, const float *d_nrm,
                                   const vrt_probe *d_probes, void *stream);

/* LightProbe::is_overlap(AABB3D{box}) on the host (box = min xyz, max xyz):
 * 1 / 0, negative on a NULL argument.  The float32 squared-distance test,
 * one rounding per operation. */
int vrt_probe_overlap(const vrt_probe *p, const float box[6]);
/* LightProbe::isect(ray, isect) on the host (VRT/voxel_octree.cc:546-554 with
 * jql::sphere_ray_isect / quadratic_solver, VRT/graphics_math.h:1105-1126,
 * 1175-1206): 1 and *t, hit_p = o + t * d on success, 0 otherwise (outputs
 * untouched).  The ray's tmin / tmax are not consulted.  The normal keeps the
 * reference's aliasing: `*isect = ISect{hit, isect->hit - o_}` reads the
 * ISect's hit point before it is overwritten, and ISect's constructor
 * normalises, so normal = normalize(prev_hit - o) with prev_hit = the hit
 * point the caller's ISect held (in a leaf: that of the last record before
 * this one whose isect succeeded, else the march's initial ISect, zero). */
int vrt_probe_isect(const vrt_probe *p, const vrt_ray *ray, const float prev_hit[3],
                    float *t, float hit_p[3], float normal[3]);

/* gi::ray_march's last parameter.  flags == 0, or a scene without probes:
 * vrt_ray_march_batch.  VRT_MARCH_EVEN_INVISIBLE on a probe scene:
 * ray_march(root, ray, .., true) -- probes are tested after a leaf's
 * triangles, ray_march_isect's first minimum runs over the whole list, and a
 * probe hit has tri = ntri + k, hit_p / normal as vrt_probe_isect. */
#define VRT_MARCH_EVEN_INVISIBLE 1
int vrt_ray_march_batch_ex(vrt_scene *s, const vrt_ray *rays, int64_t n, int flags, vrt_hit *hits);
int vrt_ray_march_batch_ex_device(vrt_scene *s, const vrt_ray *d_rays, int64_t n, int flags,
                                  vrt_hit *d_hits, void *stream);

/* trace() on a probe scene.  vrt_trace_batch[_device] restate trace(root, ray,
 * 5, true) (VRT/main.cc:10-30), whose ray_march passes even_invisible = true:
 * on a probe scene they run the mixed march.  A triangle hit is shaded as on
 * any scene (the cone march and the direct term read the probe scene's light
 * map, in which a leaf holding only probes has coverage 1,
 * VRT/voxel_octree.cc:192-199).  A probe hit returns get_albedo(isect) =
 * LightProbe::eval(normalize(hit - o_)) over the scene's stored SGs
 * (VRT/voxel_octree.cc:562-566, VRT/main.cc:25-29); parts->indirect and
 * parts->direct are +0 there (the reference computes and discards them) and
 * parts->albedo equals rgb.  eval needs the C library's expf (vrt_probe_eval's
 * pinned contract), so the host-array call fills those elements on the host
 * after the device pass; the device call writes +0 to rgb and to every part
 * there and marks the element through hits[i].tri >= ntri.
 * vrt_probe_shade_hits finishes such a batch on the host to the host call's
 * bytes: for every element of `hits` (host array; a device caller copies back
 * what it passed as d_parts->hits) that ended on a probe it writes the colour
 * to rgb[3i..] and albedo[3i..] (host arrays, either may be NULL) and leaves
 * every other element untouched. */
int vrt_probe_shade_hits(vrt_scene *s, const vrt_hit *hits, int64_t n, float *rgb, float *albedo);

/* ---- probe hits shaded on the device -------------------------------------
 * LightProbe::eval calls the C library's expf.  The kernels compute the same
 * bits with a model of it: glibc's table-driven single-precision expf
 * restated in fp64, in two flavours -- 0: every operation rounded on its own
 * (glibc's generic build), 1: the argument reduction r = fma(InvLn2N, x, -kd)
 * fused (glibc's FMA build).  vrt_expf_flavour reports which one this
 * process's expf is, found once by comparing expf with both flavours at about
 * 64 K inputs (every binade of [2^-27, 128) for both signs, the special-case
 * boundaries and the two inputs at which the flavours differ): 0, 1, or -1 for
 * a libm that is neither.  With -1 every device-shading call below returns
 * VRT_E_INVALID; vrt_trace_batch and vrt_probe_shade_hits remain the way on
 * the host. */
int vrt_expf_flavour(int *flavour);
/* The host model: y[i] = the model's expf(x[i]), flavour 0 or 1. */
int vrt_expf_model(const float *x, int64_t n, int flavour, float *y);
/* The kernels' model on `device` over host arrays (for comparing the device
 * with vrt_expf_model; either flavour, whatever this process's expf is). */
int vrt_expf_model_device(int device, const float *x, int64_t n, int flavour, float *y);
/* The model against this process's expf on the float bit patterns first_bits
 * + k * stride, k < count (32-bit wrap-around; NaN inputs are skipped):
 * *mismatches = the patterns whose results differ in bits, *first_bad = the
 * first such pattern in k order (untouched when there is none; may be NULL).
 * device < 0: the host model on up to 16 threads; device >= 0: the kernels'
 * model on that device, chunk by chunk, compared on the host. */
int vrt_expf_selftest(int device, uint32_t first_bits, uint64_t count, uint32_t stride, int flavour,
                      uint64_t *mismatches, uint32_t *first_bad);

/* vrt_probe_eval on device arrays (d_sgs: 14 n records, d_dirs: m x 3,
 * d_rgb: n x m x 3), enqueued on `stream`: the same float operations with the
 * model's expf of the detected flavour, so the same bytes (a NaN result is NaN
 * on both, its sign bit may differ). */
int vrt_probe_eval_device(int device, const vrt_sg *d_sgs, int64_t n, const float *d_dirs, int64_t m,
                          float *d_rgb, void *stream);
/* vrt_probe_shade_hits where the batch lies: d_hits, d_rgb, d_albedo are the
 * device arrays a vrt_trace_batch_device call wrote (either of the last two
 * may be NULL).  Elements that ended on a probe receive
 * eval(normalize(hit_p - o)) over the scene's stored SGs; every other element
 * is left untouched.  No host synchronisation; ordered on `stream` behind the
 * scene's work in flight. */
int vrt_probe_shade_hits_device(vrt_scene *s, const vrt_hit *d_hits, int64_t n, float *d_rgb, float *d_albedo,
                                void *stream);

/* ---- the SG algebra (VRT/voxel_octree.cc:497-528) --------------------------
 * gi::SG's constructor, SG::integral, gi::prod and gi::inner_prod, batched:
 * element i of every output comes from element i of the inputs.  Records are
 * used as they are (nothing is re-normalised on input, as vrt_probe_eval).
 * Everything is float32 with one rounding per operation in the reference's
 * order: jql::dot a sequential sum from zero, jql::length = sqrtf(dot),
 * `2 * jql::pi` formed first with jql::pi the float, SG::integral's
 * unqualified exp the float expf.  Non-finite results are the reference's
 * (sharpness 0 gives inf * 0 = NaN); a NaN's sign bit is not specified.
 * n == 0 is VRT_OK and touches nothing; n < 0 or a NULL array is
 * VRT_E_INVALID.  The host calls use the C library's expf. */
/* SG{a, d, s}: out[i] = {a, d / length(d), s}.  a, d: 3n floats, s: n. */
int vrt_sg_make(const float *a, const float *d, const float *s, int64_t n, vrt_sg *out);
/* SG::integral: rgb[3i..] = 2 * pi * (a / s) * (1.0f - expf(-2.0f * s)) */
int vrt_sg_integral(const vrt_sg *sgs, int64_t n, float *rgb /* 3n */);
/* gi::prod: with d = (lhs.s * lhs.d + rhs.s * rhs.d) / lm, lm = lhs.s + rhs.s
 * and dl = length(d): out[i] = SG{lhs.a * rhs.a * expf(lm * (dl - 1)), d,
 * lm * dl} through the constructor (axis d / length(d)) */
int vrt_sg_prod(const vrt_sg *lhs, const vrt_sg *rhs, int64_t n, vrt_sg *out);
/* gi::inner_prod: with uml = length(lhs.s * lhs.d + rhs.s * rhs.d):
 * rgb[3i..] = (2.0f * pi * (expf(uml - lhs.s - rhs.s) * lhs.a * rhs.a) *
 * (1.0f - expf(-2.0f * uml))) / uml */
int vrt_sg_inner_prod(const vrt_sg *lhs, const vrt_sg *rhs, int64_t n, float *rgb /* 3n */);
/* The same over device arrays on `device`, enqueued on `stream` with no host
 * synchronisation: the same float operations with the model's expf of the
 * detected flavour (vrt_expf_flavour; -1: VRT_E_INVALID), so the host calls'
 * bytes. */
int vrt_sg_integral_device(int device, const vrt_sg *d_sgs, int64_t n, float *d_rgb, void *stream);
int vrt_sg_prod_device(int device, const vrt_sg *d_lhs, const vrt_sg *d_rhs, int64_t n, vrt_sg *d_out,
                       void *stream);
int vrt_sg_inner_prod_device(int device, const vrt_sg *d_lhs, const vrt_sg *d_rhs, int64_t n, float *d_rgb,
                             void *stream);

/* ---- the light a scene's probes send to a point ---------------------------
 * For element i, with p = isects[i].hit_p and the lobe q = SG{lobe_a,
 * isects[i].normal, lobe_s} through the constructor (a zero normal gives a
 * NaN axis, as the reference's would):
 *  - p outside the root box (min <= p <= max on every axis; a NaN fails):
 *    count = 0, rgb = +0.
 *  - Otherwise the leaf of p: from the root, child 4 * (p.x > c.x) + 2 *
 *    (p.y > c.y) + (p.z > c.z) with c = aabb.center() = (min + max) * .5f,
 *    gi::cone_trace's descent (VRT/voxel_octree.cc:261-269) without its level
 *    limit.  A leaf above max_depth or without probes: count = 0, rgb = +0.
 *  - acc = 0; for each probe k of the leaf's probe list in list order
 *    (vrt_scene_probe_leaves'), for its lobes j = 0..13 in order: acc +=
 *    inner_prod(stored SG 14 k + j, q), componentwise; rgb = acc /
 *    (float)count, count = the list's length: the plain mean, the shape of
 *    gather_light's litness /= (float)size.
 * The stored SGs are vrt_scene_probe_sgs'; no light map is needed.  lobe_a
 * (float[3]) and lobe_s are the caller's: the two constants are the usual
 * one-lobe fit of a clamped cosine.  count (n, may be NULL) receives the list
 * lengths.  n == 0 is VRT_OK and touches nothing.  VRT_E_INVALID on a scene
 * without probes, n < 0 or a NULL isects / lobe_a / rgb.
 * The host-array call runs on the host, from the scene's host arrays and the
 * C library's expf, on a device scene and on a host-only one alike (it first
 * fetches the stored SGs if a device gather wrote them last).  The device call
 * (device arrays; VRT_E_NODEVICE on a host-only scene, VRT_E_INVALID with
 * expf flavour -1) is enqueued on `stream` with no host synchronisation,
 * ordered behind the scene's work in flight as vrt_probe_shade_hits_device
 * is, reads the stored SGs current in stream order, and gives the host
 * call's bytes. */
#define VRT_SG_COSINE_AMPLITUDE 1.17f
#define VRT_SG_COSINE_SHARPNESS 2.133f
int vrt_probe_irradiance(vrt_scene *s, const vrt_isect *isects, int64_t n, const float lobe_a[3], float lobe_s,
                         float *rgb /* 3n */, int32_t *count /* n, may be NULL */);
int vrt_probe_irradiance_device(vrt_scene *s, const vrt_isect *d_isects, int64_t n, const float lobe_a[3],
                                float lobe_s, float *d_rgb, int32_t *d_count, void *stream);

/* trace() frames of a probe scene (VRT/main.cc:10-30 with the probe block of
 * :104-105 in place): vrt_render_trace, vrt_render_trace_device and
 * vrt_trace_frame_device argument for argument, with the mixed march as the
 * primary pass and a probe hit coloured by LightProbe::eval over the stored
 * SGs (no cones, no direct term).  s_hit is 0 for a miss, 1 for a triangle, 2
 * for a probe.  On a scene without probes they are the old calls.
 * vrt_trace_frame_probes_device: light_color (float[3]) given, the scene's
 * probes gather behind the filter (vrt_scene_probes_gather's values) before
 * the view is shaded; NULL keeps the stored SGs. */
int vrt_render_trace_probes(vrt_scene *s, const vrt_camera *cam, const vrt_film *film, float min_voxel,
                            float *rgb, int32_t *s_hit, float *s_rgb);
int vrt_render_trace_probes_device(vrt_scene *s, const vrt_camera *cam, const vrt_film *film,
                                   float min_voxel, int rank, int nranks, int image_layout,
                                   float *d_out, void *stream);
int vrt_trace_frame_probes_device(vrt_scene *s, const vrt_camera *light_cam, const vrt_film *light_film,
                                  const float *light_color, const vrt_camera *cam, const vrt_film *film,
                                  float min_voxel, int rank, int nranks, int image_layout, float *d_out,
                                  void *stream, int64_t *hits);

/* ---- trace() frames and probe scenes on the multi-device handle -----------
 * vrt_scene_create_multi with light probes: flags as vrt_scene_create_probes
 * (0 builds on the host, VRT_BUILD_DEVICE | VRT_BUILD_DEVICE_PROBES on rank
 * 0's device, anything else is VRT_E_INVALID), checked after the mask and the
 * devices' visibility as vrt_scene_create_multi checks its own.  Every replica
 * holds rank 0's probes, probe lists and masks and stored SGs.  nprobe == 0 or
 * probes == NULL is vrt_scene_create_multi.  vrt_multi_set_probe_sgs:
 * vrt_scene_set_probe_sgs (14 * nprobe records) on every rank. */
int vrt_scene_create_multi_probes(const vrt_scene_desc *desc, const vrt_probe *probes, int32_t nprobe,
                                  int max_depth, uint32_t device_mask, int flags, vrt_multi **out);
int vrt_multi_set_probe_sgs(vrt_multi *m, const vrt_sg *sgs);

/* ---- moving a multi-device scene (the vrt_multi handle) --------------------
 * vrt_scene_update / vrt_scene_update_probes for every rank of a handle at
 * once, so that the ranks stay replicas.  pos is required (ntri*9); nrm is
 * optional (NULL: the stored normals stay); probes (nprobe records) is
 * optional on a handle made by vrt_scene_create_multi_probes with probes
 * (NULL: the probes stay where they are) and VRT_E_INVALID on any other.  On
 * success every rank's scene equals, bit for bit, the same rank's scene of a
 * handle freshly created from these arrays with VRT_BUILD_DEVICE (| VRT_BUILD_
 * DEVICE_PROBES), whichever flags this handle was created with: every query,
 * march, render and device array, and the host copy of the probes.  Derived
 * state is a fresh scene's on every rank (no light map: vrt_render_trace_
 * multi* return VRT_E_INVALID until vrt_lightmap_build_multi or
 * vrt_trace_frame_multi* runs).  What the handle owns stays: communicator,
 * streams, events, send / gather buffers, config-5 scratch, the image pair,
 * the light mode, each rank scene's frames-in-flight hint, queues, scratch and
 * update scratch, and the stored SGs on every rank.  Waiting and thread rules
 * are vrt_scene_update's, per device; the call returns when every rank is
 * ready, and the caller may then overwrite the arrays.
 * All ranks or none: every rank first does everything that can refuse (bad
 * arguments, a bad probe, a size limit of the build, no host or device memory:
 * VRT_E_INVALID, VRT_E_NOMEM, or VRT_E_DEVICE from an allocation; the text
 * names the rank and its device), and only when no rank refused is any array
 * that a frame reads written on any rank.  A refusal leaves every rank on its
 * previous geometry and probes, fully usable.  Only a failed launch or copy
 * after that point (VRT_E_DEVICE) can leave the handle half rebuilt: destroy
 * it then.
 * flags: 0, or VRT_MULTI_UPDATE_VERIFY: after the update every rank computes
 * vrt_scene_digest on its stream and the host compares the ten words of every
 * rank, its vrt_scene_info counts, record format, root box and chain spacing
 * with rank 0's; a difference is VRT_E_DEVICE "replicas diverged: rank %d
 * (device %d), <item>".  Other bits are VRT_E_INVALID. */
#define VRT_MULTI_UPDATE_VERIFY 1
int vrt_multi_update(vrt_multi *m, const float *pos, const float *nrm, const vrt_probe *probes, int flags);
/* The same from arrays on rank 0's device, read in `stream` order (a stream of
 * that device; NULL = its null stream) and distributed to the other ranks by
 * one ncclBroadcast per array (virtual ranks: device copies).  d_probes needs
 * only a float's alignment.  A bad probe is found by the root-box kernel and
 * reported as VRT_E_INVALID with its index. */
int vrt_multi_update_device(vrt_multi *m, const float *d_pos, const float *d_nrm, const vrt_probe *d_probes,
                            int flags, void *stream);
/* The last successful update's wall-clock split: {total, the slowest rank's
 * own vrt_scene_update_stats total, distribution of device arrays to ranks
 * >= 1 (events on rank 0's stream; 0 for host arrays and for one rank), verify
 * (0 without the flag)}.  VRT_E_INVALID before the first update. */
int vrt_multi_update_stats(const vrt_multi *m, double ms[4]);

/* How the ranks share a light-map build.  REPLICATED (the default): every rank
 * marches the whole light film.  SHARDED: rank i marches its tiles of the
 * light film's tile deal (the view's deal, vrt_tile_deal_map), the ranks
 * exchange their hit lists (RCCL on each rank's scene stream), and every rank
 * sorts and sums the union: a hit's key holds its index in the canonical
 * order, which does not depend on who marched it, so every rank ends with the
 * single-device light map, bit for bit, in either mode.  After a sharded build
 * vrt_lightmap_stats on a rank's scene reports that rank's share.  A 1-rank
 * handle builds the whole map in either mode.  Other values: VRT_E_INVALID. */
#define VRT_MULTI_LIGHT_REPLICATED 0
#define VRT_MULTI_LIGHT_SHARDED 1
int vrt_multi_set_light_mode(vrt_multi *m, int mode);
/* The light map on every rank (vrt_lightmap_build's values); *hits (may be
 * NULL) is the light pass's hit count: in sharded mode the sum of the ranks',
 * in replicated mode every rank's own, which must agree (VRT_E_DEVICE if the
 * replicas diverged).  Returns when every rank's map is built. */
int vrt_lightmap_build_multi(vrt_multi *m, const vrt_camera *light_cam, const vrt_film *light_film, int64_t *hits);
/* The cone-traced view over the ranks' current light maps (VRT_E_INVALID
 * unless every rank has one): rank i shades its tiles of the deal, packed
 * tile-major, then the gather and unpack of vrt_render_multi.  The image
 * (nx*ny*3, index y*nx+x, zero outside the tile grid) is vrt_render_trace's
 * bit for bit, for any rank count; on a probe handle, vrt_render_trace_probes'.
 * Host array, or d_image on rank 0's device with the stream ordering of
 * vrt_render_multi_device. */
int vrt_render_trace_multi(vrt_multi *m, const vrt_camera *cam, const vrt_film *film, float min_voxel, float *rgb);
int vrt_render_trace_multi_device(vrt_multi *m, const vrt_camera *cam, const vrt_film *film, float min_voxel,
                                  float *d_image, void *stream);
/* The reference main() frame in one call: the light-map build above and,
 * beside each rank's light march, the primary march of its share of the view.
 * The light march is enqueued on every rank before the host waits for any
 * rank's hit count (one sync per rank).  On a probe handle each rank's work is
 * vrt_trace_frame_probes_device's: with light_color (float[3]) every rank
 * gathers the scene's probes behind the filter (identical SGs everywhere),
 * with NULL the stored SGs are kept; without probes light_color is ignored.
 * Arguments are checked as the per-rank calls check them, before anything is
 * enqueued; after a failure on any rank nothing collective is enqueued and
 * every rank's streams are synchronised before the error is returned. */
int vrt_trace_frame_multi(vrt_multi *m, const vrt_camera *light_cam, const vrt_film *light_film,
                          const float *light_color, const vrt_camera *cam, const vrt_film *film,
                          float min_voxel, float *rgb, int64_t *hits);
int vrt_trace_frame_multi_device(vrt_multi *m, const vrt_camera *light_cam, const vrt_film *light_film,
                                 const float *light_color, const vrt_camera *cam, const vrt_film *film,
                                 float min_voxel, float *d_image, void *stream, int64_t *hits);
/* The three calls above with a light list (vrt_lightmap_build_lights).
 * Replicated: every rank marches every light's whole film.  Sharded: rank i
 * marches its tiles of each light film's own tile deal; a key's canonical
 * index runs over the samples of all lights, so the exchanged lists merge as
 * one light's do.  Every rank ends with the single-device map bit for bit.
 * *hits: the total over all lights.  probe_light_color: the light_color of
 * vrt_trace_frame_multi (the probes' gather on a miss), not a light's colour.
 * Arguments are checked before anything is enqueued, as above. */
int vrt_lightmap_build_lights_multi(vrt_multi *m, const vrt_light *lights, int nlights, int64_t *hits);
int vrt_trace_frame_lights_multi(vrt_multi *m, const vrt_light *lights, int nlights,
                                 const float *probe_light_color, const vrt_camera *cam,
                                 const vrt_film *film, float min_voxel, float *rgb, int64_t *hits);
int vrt_trace_frame_lights_multi_device(vrt_multi *m, const vrt_light *lights, int nlights,
                                        const float *probe_light_color, const vrt_camera *cam,
                                        const vrt_film *film, float min_voxel, float *d_image, void *stream,
                                        int64_t *hits);

/* Config 5 over the handle's ranks: rank i renders its share
 * (vrt_render_secondary_tiles_device) on its stream into scratch the handle
 * owns, one gather of tiles_per_rank * 64 floats per rank to rank 0,
 * vrt_unpack_tiles_c_device (comps = 1) there.  vis (nx*ny floats, index
 * y*nx+x, zero outside the tile grid) is vrt_render_secondary's, bit for bit,
 * for any rank count; *rays (may be NULL) = 8*(nx/8)*8*(ny/8) + spp * (sum of
 * the ranks' primary hits) = vrt_render_secondary's *rays.  spp outside 1..64,
 * a bad film or a NULL argument: VRT_E_INVALID before anything is enqueued;
 * after a failure on any rank nothing collective is enqueued and every rank's
 * streams are synchronised.  A probe handle skips the probes. */
int vrt_render_secondary_multi(vrt_multi *m, const vrt_camera *cam, const vrt_film *film, int spp,
                               float *vis, int64_t *rays);
/* d_vis on rank 0's device, stream ordering as vrt_render_multi_device. */
int vrt_render_secondary_multi_device(vrt_multi *m, const vrt_camera *cam, const vrt_film *film, int spp,
                                      float *d_vis, void *stream);

/* ---- output (VRT/stb_image_write.h:178,723-757) ------------------------- */
/* Byte-identical to stbi_write_hdr: returns 1 on success, 0 on failure. */
int vrt_write_hdr(const char *filename, int w, int h, int comp,
                  const float *data);
/* Same bytes into memory: returns the byte count, or -(needed) if cap is
 * too small, or 0 on invalid input. */
int64_t vrt_write_hdr_mem(int w, int h, int comp, const float *data,
                          uint8_t *out, int64_t cap);

/* Device half of the writer: stbiw__linear_to_rgbe for every pixel of a
 * device image (w*h*comp floats) into w*h*4 device bytes on `stream`; then
 * vrt_write_hdr_rgbe[_mem] RLE-encodes those bytes on the host.  The file is
 * byte-identical to vrt_write_hdr / stbi_write_hdr on the same pixels. */
int vrt_rgbe_device(const float *d_img, int w, int h, int comp,
                    uint8_t *d_rgbe, void *stream);
int vrt_write_hdr_rgbe(const char *filename, int w, int h,
                       const uint8_t *rgbe);
int64_t vrt_write_hdr_rgbe_mem(int w, int h, const uint8_t *rgbe,
                               uint8_t *out, int64_t cap);

/* ---- legacy reference symbols (identical signatures and results) ------- */
/* C linkage here; the library also defines the same two functions with the
 * reference headers' C++ linkage (declared in vrt_legacy.hpp), the names
 * VRT/voxel_octree.cc:446,490 import. */
/* VRT/raytri.h:5-7 */
int intersect_triangle3(double orig[3], double dir[3], double vert0[3],
                        double vert1[3], double vert2[3], double *t,
                        double *u, double *v);
/* VRT/tribox2.h:6 */
int triBoxOverlap(float boxcenter[3], float boxhalfsize[3],
                  float triverts[3][3]);
/* VRT/stb_image_write.h:178 (stb_image_write v1.13, called at VRT/main.cc:126):
 * the same function as vrt_write_hdr, under the reference's name, so a
 * caller of the reference's writer relinks without renaming the call. */
int stbi_write_hdr(char const *filename, int w, int h, int comp,
                   const float *data);

/* ---- build identity ---------------------------------------------------- */
/* Source hash this library was built from (tools/build_id.py: sha256 of
 * csrc/, include/vrt.h and the Makefile, 16 hex digits). */
const char *vrt_build_id(void);
/* The value of one path-selecting compile-time switch of this build (e.g.
 * "VRT_SEC_SPILL_T": config 5's compaction threshold, 0 = no compaction;
 * "VRT_SEC_SLICE_CHUNK", "VRT_SLICE_CHUNK": the persistent kernels' slice
 * chunks; "VRT_SEC_TAKE": config-5 pixels per dequeue; "VRT_DEAL_BLOCK" / "VRT_DEAL_WEIGHT" / "VRT_DEAL_SPAN": the tile
 * deal; "VRT_LIGHT_BUDGET" / "VRT_PRIM_BUDGET": the trace walks' budgets);
 * VRT_E_INVALID for a name the build does not know.  Lets a test assert which
 * path a build takes. */
int vrt_build_flag(const char *name, int64_t *value);

/* ---- scene ingest (VRT/voxel_octree.cc:305-388) -------------------------
 * vrt_obj_load = obj2voxel(path) + load_image for every texture a face
 * uses: tinyobjloader v1.4.0 LoadObj(.., path, mtldir = dir(path) + "/",
 * triangulate = true) restated bit-exactly (its non-correctly-rounded float
 * parser and ear-clipping triangulation included), then one triangle per
 * (shape, face) in shape order.  Textures are decoded like stbi_load(path,
 * .., 0) (TGA only).  Faces without normals or with out-of-range indices
 * are errors; faces without a material get an extra default material (Kd
 * 0) appended after the file's materials.  VRT_OBJ_PARSE_ONLY stops after
 * LoadObj (no soup, no textures; no normal requirement). */
#define VRT_OBJ_PARSE_ONLY 1

typedef struct vrt_obj vrt_obj;
typedef struct {
        int64_t nvert, nnormal, ntexcoord; /* attrib_t sizes / 3, / 3, / 2 */
        int32_t nshape;                    /* shapes.size() */
        int64_t nface;                     /* triangles over all shapes */
        int32_t nmat;                      /* materials.size() (MTL order) */
        int32_t has_soup;                  /* 0 with VRT_OBJ_PARSE_ONLY */
        int32_t nsoup_mat;                 /* nmat (+1 if a default was added) */
        int32_t ntex;
        int64_t tex_bytes;
} vrt_obj_info_t;

int vrt_obj_load(const char *obj_path, int flags, vrt_obj **out);
void vrt_obj_free(vrt_obj *o);
int vrt_obj_info(const vrt_obj *o, vrt_obj_info_t *info);
/* Borrowed views, valid until vrt_obj_free: attrib_t::vertices / normals /
 * texcoords. */
int vrt_obj_attrib(const vrt_obj *o, const float **v, const float **vn,
                   const float **vt);
/* Per triangle (shape order): idx[9] = {v, vn, vt} x 3 (0-based, -1 =
 * absent), tinyobj material id (-1 = none) and shape index.  Any output may
 * be NULL; sizes from vrt_obj_info().nface. */
int vrt_obj_faces(const vrt_obj *o, int32_t *idx, int32_t *mat,
                  int32_t *shape);
/* material_t i: name, diffuse (Kd), diffuse_texname (as in the MTL). */
int vrt_obj_material(const vrt_obj *o, int i, const char **name, float kd[3],
                     const char **texname);
/* Resolved file of soup texture i (mtldir + diffuse_texname). */
int vrt_obj_texture_path(const vrt_obj *o, int i, const char **path);
const char *vrt_obj_warnings(const vrt_obj *o);
/* The soup as a scene descriptor for vrt_scene_create (borrowed pointers). */
int vrt_obj_scene_desc(const vrt_obj *o, vrt_scene_desc *desc);

/* stbi_load(path, &w, &h, &comp, 0) for TGA files (VRT/stb_image.h:
 * 5404-5640): 8-bit interleaved, row 0 = top; free with vrt_image_free. */
int vrt_tga_load(const char *path, int *w, int *h, int *comp, uint8_t **out);
int vrt_tga_decode(const uint8_t *buf, int64_t len, int *w, int *h, int *comp,
                   uint8_t **out);
void vrt_image_free(uint8_t *p);

/* ---- synthetic inputs ----------------------------------------------------
 * Deterministic "sponza-proxy" atrium (no Sponza asset ships): floor, walls,
 * two storeys of colonnades and arches, curtains, details; every material
 * textured with procedural 8-bit textures.  `detail` scales tessellation
 * (1.0 ~ 262k triangles).  Two-call protocol: call with NULL arrays to get
 * counts in *ntri / *nmat / *ntex / *tex_bytes, then with arrays sized to
 * them.  Bounds match the scaled Sponza frame the reference cameras use
 * (VRT/main.cc:76-78,112-115). */
int vrt_proxy_scene(double detail, uint32_t seed, int32_t *ntri, float *pos,
                    float *nrm, float *uv, int32_t *mat, int32_t *nmat,
                    int32_t *mat_tex, float *mat_kd, int32_t *ntex,
                    int32_t *tex_dims, int64_t *tex_off, uint8_t *tex_data,
                    int64_t *tex_bytes);
/* Camera-sweep pose i of n: ellipse at 0.4 * AABB height around the AABB
 * centre, looking at the centre, fov 90 degrees. */
int vrt_sweep_pose(const float root_min[3], const float root_max[3], int i,
                   int n, float eye[3], float spot[3], float up[3],
                   float *fov);

const char *vrt_status_string(int status);
const char *vrt_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
