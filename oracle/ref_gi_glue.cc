// ref_gi_glue.cc -- TEST INFRASTRUCTURE ONLY.
//
// C-linkage entry points onto the reference's own camera.cc and
// voxel_octree.cc, which oracle/Makefile compiles unmodified, in place, into
// oracle/_ref/libvrtref_gi.so (never shipped, never loaded by the product).
// Nothing here re-implements reference behaviour: every function builds the
// reference's own objects from flat arrays, calls the reference, and copies
// the result out.  Where the reference's main() holds a loop of its own (the
// light block, VRT/main.cc:80-97), the loop here only fixes the order the
// reference's thread pool leaves open ("light map") and calls the
// same reference functions per sample.
#include "voxel_octree.h"
#include "camera.h"

#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

// Functions the reference defines in voxel_octree.cc without declaring them
// in its header.
namespace gi
{
void split(VoxelOctree* root);
void travorder(const VoxelOctree& root, const jql::Ray& ray, int ord[8]);
}

// LightProbe keeps its SGs private and offers no accessor; an explicit
// instantiation may name a private member, which gives one without touching
// the class.
gi::SG (&rgi_sgs(gi::LightProbe& p))[14];
template <gi::SG (gi::LightProbe::*M)[14]>
struct rgi_rob {
        friend gi::SG (&rgi_sgs(gi::LightProbe& p))[14]
        {
                return p.*M;
        }
};
template struct rgi_rob<&gi::LightProbe::sgs_>;

namespace
{
Vec3 v3(const float* p)
{
        return Vec3{ p[0], p[1], p[2] };
}

void put3(float* p, const Vec3& v)
{
        p[0] = v.x;
        p[1] = v.y;
        p[2] = v.z;
}

// a ray taken as it is (the Ray constructor would normalise d again)
Ray raw_ray(const float* r)
{
        Ray ray;
        ray.o = v3(r);
        ray.d = v3(r + 3);
        ray.tmin = r[6];
        ray.tmax = r[7];
        return ray;
}

ISect raw_isect(const float* q)
{
        ISect is;
        is.hit = v3(q);
        is.normal = v3(q + 3);
        return is;
}

gi::SG raw_sg(const float* q)
{
        gi::SG g;
        g.a = v3(q);
        g.d = v3(q + 3);
        g.s = q[6];
        return g;
}

void put_sg(float* q, const gi::SG& g)
{
        put3(q, g.a);
        put3(q + 3, g.d);
        q[6] = g.s;
}

struct Scene {
        std::vector<tinyobj::material_t> materials;
        std::vector<gi::Triangle> tris;
        std::vector<gi::LightProbe> probes;
        std::vector<gi::VoxelBase*> voxels;
        gi::VoxelOctree root;
        // leaf -> ix | iy << 10 | iz << 20 at its depth (child i: x high iff
        // i & 4, y: i & 2, z: i & 1), the oracle's voxel code
        std::unordered_map<const gi::VoxelOctree*, uint32_t> code;
        int64_t nodes = 0, refs = 0;

        int64_t index_of(const gi::VoxelBase* v) const
        {
                auto* t = dynamic_cast<const gi::Triangle*>(v);
                if (t)
                        return t - tris.data();
                auto* p = dynamic_cast<const gi::LightProbe*>(v);
                return (int64_t)tris.size() + (p - probes.data());
        }
};

void walk_codes(Scene* s, const gi::VoxelOctree* n, uint32_t x, uint32_t y, uint32_t z)
{
        s->nodes++;
        s->refs += (int64_t)n->voxels.size();
        s->code[n] = x | (y << 10) | (z << 20);
        if (!n->children[0])
                return;
        for (uint32_t i = 0; i < 8; ++i)
                walk_codes(s, n->children[i].get(), 2 * x + ((i >> 2) & 1), 2 * y + ((i >> 1) & 1), 2 * z + (i & 1));
}

struct Dump {
        uint64_t* key;
        int32_t* leaf;
        float* box;
        float* cov;
        float* illum;
        int32_t* cnt;
        int32_t* vox;
        int64_t n = 0, r = 0;
};

void walk_dump(const Scene* s, const gi::VoxelOctree* n, int depth, Dump* d)
{
        int64_t i = d->n++;
        d->key[i] = ((uint64_t)depth << 32) | s->code.at(n);
        d->leaf[i] = n->children[0] ? 0 : 1;
        put3(d->box + 6 * i, n->aabb.min);
        put3(d->box + 6 * i + 3, n->aabb.max);
        d->cov[i] = n->coverage;
        for (int f = 0; f < 6; ++f)
                put3(d->illum + 18 * i + 3 * f, n->illum[f]);
        d->cnt[i] = (int32_t)n->voxels.size();
        for (auto* v : n->voxels)
                d->vox[d->r++] = (int32_t)s->index_of(v);
        if (!n->children[0])
                return;
        for (int c = 0; c < 8; ++c)
                walk_dump(s, n->children[c].get(), depth + 1, d);
}

// One sample of the light block: what a hit adds to its leaf, face by face
// (the weight is the clamped cosine between the face's axis and the normal).
int deposit(Scene* s, const Ray& ray, const Vec3& light_color)
{
        gi::VoxelOctree* leaf = nullptr;
        gi::VoxelBase* voxel = nullptr;
        ISect isect{};
        if (!gi::ray_march(&s->root, ray, &leaf, &voxel, &isect))
                return 0;
        const Vec3 lit = voxel->get_diffuse(isect, ray, light_color);
        for (int face = 0; face < 6; ++face) {
                const float w = jql::clamp(jql::dot(gi::VoxelOctree::illum_d[face], isect.normal), 0.f, 1.f);
                leaf->illum[face] += w * lit;
        }
        return 1;
}

Camera make_camera(const float* cam)
{
        // cam: fov, eye[3], spot[3], up[3], near, far
        return Camera{ cam[0], v3(cam + 1), v3(cam + 4), v3(cam + 7), cam[10], cam[11] };
}
}

extern "C" {

// ---- scene -------------------------------------------------------------------
// pos / nrm: ntri * 9, uv: ntri * 6, mat: ntri ids into kd (nmat * 3) and
// texname (nmat strings; empty or NULL: untextured, else a file the
// reference's texel_fetch loads).  probes: nprobe * 4 {o, r}, pushed behind
// the triangles as VRT/main.cc:56-64 does.
void* rgi_scene_create(const float* pos, const float* nrm, const float* uv, const int32_t* mat, int ntri, int nmat,
                       const float* kd, const char* const* texname, const float* probes, int nprobe, int max_depth)
{
        auto* s = new Scene;
        s->materials.resize(nmat);
        for (int m = 0; m < nmat; ++m) {
                std::memcpy(s->materials[m].diffuse, kd + 3 * m, 3 * sizeof(float));
                if (texname && texname[m])
                        s->materials[m].diffuse_texname = texname[m];
        }
        s->tris.reserve(ntri);
        for (int t = 0; t < ntri; ++t) {
                const float *p = pos + 9 * t, *n = nrm + 9 * t, *u = uv + 6 * t;
                s->tris.emplace_back(v3(p), v3(p + 3), v3(p + 6), v3(n), v3(n + 3), v3(n + 6), Vec2{ u[0], u[1] },
                                     Vec2{ u[2], u[3] }, Vec2{ u[4], u[5] }, &s->materials[mat[t]]);
        }
        s->probes.reserve(nprobe);
        for (int k = 0; k < nprobe; ++k)
                s->probes.emplace_back(v3(probes + 4 * k), probes[4 * k + 3]);
        for (auto& t : s->tris)
                s->voxels.push_back(&t);
        for (auto& p : s->probes)
                s->voxels.push_back(&p);
        gi::ray_march_init(&s->root, s->voxels, max_depth);
        walk_codes(s, &s->root, 0, 0, 0);
        return s;
}

void rgi_scene_destroy(void* h)
{
        delete static_cast<Scene*>(h);
}

// info[0] = nodes, info[1] = length of all nodes' voxel lists
void rgi_tree_info(const void* h, int64_t info[2])
{
        auto* s = static_cast<const Scene*>(h);
        info[0] = s->nodes;
        info[1] = s->refs;
}

// Per node, children 0..7 in order below their parent: key = depth << 32 |
// code (root depth 1), leaf flag, aabb {min, max}, coverage, illum[6][3], the
// length of its voxel list; vox: the lists one after another, in list order.
void rgi_tree_dump(const void* h, uint64_t* key, int32_t* leaf, float* box, float* cov, float* illum, int32_t* cnt,
                   int32_t* vox)
{
        auto* s = static_cast<const Scene*>(h);
        Dump d{ key, leaf, box, cov, illum, cnt, vox };
        walk_dump(s, &s->root, 1, &d);
}

// ---- camera --------------------------------------------------------------------
// Camera::gen_rays1 / gen_rays4 on every pixel of Film(film_w, film_h, nx, ny):
// out[((py * nx + px) * k + s) * 8] = {o, d, tmin, tmax}, k = 1 or 4.
void rgi_gen_rays(const float cam[12], int four, float film_w, float film_h, int nx, int ny, float* out)
{
        Camera c = make_camera(cam);
        Film film(film_w, film_h, nx, ny);
        for (int py = 0; py < ny; ++py) {
                for (int px = 0; px < nx; ++px) {
                        auto rays = four ? c.gen_rays4(film, px, py) : c.gen_rays1(film, px, py);
                        for (auto& r : rays) {
                                put3(out, r.o);
                                put3(out + 3, r.d);
                                out[6] = r.tmin;
                                out[7] = r.tmax;
                                out += 8;
                        }
                }
        }
}

// the Ray constructor (normalises d)
void rgi_make_ray(const float o[3], const float d[3], float tmin, float tmax, float out[8])
{
        Ray r{ v3(o), v3(d), tmin, tmax };
        put3(out, r.o);
        put3(out + 3, r.d);
        out[6] = r.tmin;
        out[7] = r.tmax;
}

// AABB3D::isect(ray, nullptr) for n (box, ray) pairs
void rgi_aabb_isect(const float* box, const float* rays, int n, int32_t* out)
{
        for (int i = 0; i < n; ++i) {
                AABB3D b{ v3(box + 6 * i), v3(box + 6 * i + 3) };
                out[i] = b.isect(raw_ray(rays + 8 * i), nullptr) ? 1 : 0;
        }
}

// gi::travorder on a node of box[i] split by gi::split, for n (box, ray) pairs;
// child[n][8][6] (may be NULL) receives the children's boxes.
void rgi_travorder(const float* box, const float* rays, int n, int32_t* ord, float* child)
{
        for (int i = 0; i < n; ++i) {
                gi::VoxelOctree node;
                node.aabb = AABB3D{ v3(box + 6 * i), v3(box + 6 * i + 3) };
                gi::split(&node);
                int o[8];
                gi::travorder(node, raw_ray(rays + 8 * i), o);
                for (int k = 0; k < 8; ++k) {
                        ord[8 * i + k] = o[k];
                        if (child) {
                                put3(child + (8 * i + k) * 6, node.children[k]->aabb.min);
                                put3(child + (8 * i + k) * 6 + 3, node.children[k]->aabb.max);
                        }
                }
        }
}

// ---- ray_march and the per-hit pieces ----------------------------------------
// gi::ray_march over n rays taken as they are, the ISect zeroed before each
// call as trace() and the light block do.  Outputs (any may be NULL):
// hit[n], voxel index by pointer difference (probe k: ntri + k; -1 on a miss),
// the leaf's code (0xFFFFFFFF on a miss), isect.hit and isect.normal, and per
// hit get_diffuse(isect, ray, color), get_albedo(isect), is_visible() and
// leaf->compute_illum(-ray.d).
void rgi_ray_march(void* h, const float* rays, int n, int even_invisible, const float color[3], int32_t* hit,
                   int32_t* vox, uint32_t* code, float* hitp, float* nrm, float* diffuse, float* albedo,
                   int32_t* visible, float* illum)
{
        auto* s = static_cast<Scene*>(h);
        for (int i = 0; i < n; ++i) {
                Ray ray = raw_ray(rays + 8 * i);
                gi::VoxelOctree* leaf{};
                gi::VoxelBase* voxel{};
                ISect isect{};
                bool got = gi::ray_march(&s->root, ray, &leaf, &voxel, &isect, even_invisible != 0);
                if (hit) hit[i] = got ? 1 : 0;
                if (vox) vox[i] = got ? (int32_t)s->index_of(voxel) : -1;
                if (code) code[i] = got ? s->code.at(leaf) : 0xFFFFFFFFu;
                Vec3 zero{};
                if (hitp) put3(hitp + 3 * i, got ? isect.hit : zero);
                if (nrm) put3(nrm + 3 * i, got ? isect.normal : zero);
                if (diffuse) put3(diffuse + 3 * i, got ? voxel->get_diffuse(isect, ray, v3(color)) : zero);
                if (albedo) put3(albedo + 3 * i, got ? voxel->get_albedo(isect) : zero);
                if (visible) visible[i] = got ? (voxel->is_visible() ? 1 : 0) : -1;
                if (illum) put3(illum + 3 * i, got ? leaf->compute_illum(-ray.d) : zero);
        }
}

// ---- the light block (VRT/main.cc:80-97), serial, in the canonical order:
// task t = tx * 8 + ty, its pixels row-major, samples 0..3.  Adds to the
// tree's illum; returns the hit count.  color is get_diffuse's last argument.
int64_t rgi_lightmap(void* h, const float cam[12], float film_w, float film_h, int nx, int ny, const float color[3])
{
        auto* s = static_cast<Scene*>(h);
        Camera light_cam = make_camera(cam);
        Film light_film(film_w, film_h, nx, ny);
        const Vec3 light_color = v3(color);
        const int tile_w = nx / 8, tile_h = ny / 8;
        int64_t hits = 0;
        for (int task = 0; task < 64; ++task) {
                const int x0 = (task / 8) * tile_w, y0 = (task % 8) * tile_h;
                for (int k = 0; k < tile_w * tile_h; ++k) {
                        const int px = x0 + k % tile_w, py = y0 + k / tile_w;
                        for (const Ray& ray : light_cam.gen_rays4(light_film, px, py))
                                hits += deposit(s, ray, light_color);
                }
        }
        return hits;
}

void rgi_lightmap_filter(void* h)
{
        gi::cone_trace_init_filter(&static_cast<Scene*>(h)->root);
}

// min component of root.aabb.size() / powf(2, levels) (VRT/main.cc:69-70)
float rgi_min_voxel(const void* h, int levels)
{
        auto* s = static_cast<const Scene*>(h);
        auto res = s->root.aabb.size() / std::powf(2.f, (float)levels);
        return *std::min_element(jql::begin(res), jql::end(res));
}

// gi::cone_trace(root, isect, min_voxel) at n {hit, normal} taken as they are
void rgi_cone_trace(const void* h, const float* isects, int n, float min_voxel, float* out)
{
        auto* s = static_cast<const Scene*>(h);
        for (int i = 0; i < n; ++i)
                put3(out + 3 * i, gi::cone_trace(s->root, raw_isect(isects + 6 * i), min_voxel));
}

// Film::add of n colours at pixels xy[n][2] into a fresh Film, then
// to_float_array (nx * ny * 3)
void rgi_film_add(float film_w, float film_h, int nx, int ny, const int32_t* xy, const float* color, int n,
                  float* out)
{
        Film film(film_w, film_h, nx, ny);
        for (int i = 0; i < n; ++i)
                film.add(xy[2 * i], xy[2 * i + 1], v3(color + 3 * i));
        auto d = film.to_float_array();
        std::memcpy(out, d.data(), d.size() * sizeof(float));
}

// ---- light probes ------------------------------------------------------------
// LightProbe{o, r}.isect(ray, &isect) with isect.hit = prev beforehand (the
// reference reads it before it writes it, VRT/voxel_octree.cc:550)
void rgi_probe_isect(const float probe[4], const float* rays, const float* prev, int n, int32_t* hit, float* out)
{
        gi::LightProbe p{ v3(probe), probe[3] };
        for (int i = 0; i < n; ++i) {
                ISect is{};
                is.hit = v3(prev + 3 * i);
                bool got = p.isect(raw_ray(rays + 8 * i), &is);
                hit[i] = got ? 1 : 0;
                put3(out + 6 * i, is.hit);
                put3(out + 6 * i + 3, is.normal);
        }
}

// LightProbe{o, r}.is_overlap(box) for n boxes
void rgi_probe_overlap(const float probe[4], const float* box, int n, int32_t* out)
{
        gi::LightProbe p{ v3(probe), probe[3] };
        for (int i = 0; i < n; ++i)
                out[i] = p.is_overlap(AABB3D{ v3(box + 6 * i), v3(box + 6 * i + 3) }) ? 1 : 0;
}

// LightProbe{o, r}.gather_light(root, res, light_dir, light_color) for n
// probes of the caller's -> sgs[n][14][7] = {a, d, s}
void rgi_probe_gather(void* h, const float* probes, int n, float res, const float light_dir[3],
                      const float light_color[3], float* sgs)
{
        auto* s = static_cast<Scene*>(h);
        for (int k = 0; k < n; ++k) {
                gi::LightProbe p{ v3(probes + 4 * k), probes[4 * k + 3] };
                p.gather_light(&s->root, res, v3(light_dir), v3(light_color));
                for (int i = 0; i < 14; ++i)
                        put_sg(sgs + (k * 14 + i) * 7, rgi_sgs(p)[i]);
        }
}

// gather_light for the scene's own probe k, kept in the probe (a later march
// with even_invisible shades its hits from them)
void rgi_scene_probe_gather(void* h, int k, float res, const float light_dir[3], const float light_color[3],
                            float* sgs)
{
        auto* s = static_cast<Scene*>(h);
        auto& p = s->probes[k];
        p.gather_light(&s->root, res, v3(light_dir), v3(light_color));
        for (int i = 0; i < 14; ++i)
                put_sg(sgs + i * 7, rgi_sgs(p)[i]);
}

// LightProbe::eval(dir) of a probe holding the given 14 SGs, on m directions
void rgi_probe_eval(const float sgs[14 * 7], const float* dirs, int m, float* out)
{
        gi::LightProbe p{ Vec3{}, 1.f };
        for (int i = 0; i < 14; ++i)
                rgi_sgs(p)[i] = raw_sg(sgs + 7 * i);
        for (int j = 0; j < m; ++j)
                put3(out + 3 * j, p.eval(v3(dirs + 3 * j)));
}

// ---- SG algebra --------------------------------------------------------------
// per pair i: lhs.eval(dir), lhs.integral(), prod(lhs, rhs), inner_prod(lhs, rhs)
void rgi_sg_ops(const float* lhs, const float* rhs, const float* dirs, int n, float* eval, float* integral,
                float* prod, float* inner)
{
        for (int i = 0; i < n; ++i) {
                gi::SG a = raw_sg(lhs + 7 * i), b = raw_sg(rhs + 7 * i);
                put3(eval + 3 * i, a.eval(v3(dirs + 3 * i)));
                put3(integral + 3 * i, a.integral());
                put_sg(prod + 7 * i, gi::prod(a, b));
                put3(inner + 3 * i, gi::inner_prod(a, b));
        }
}

// the SG constructor (normalises d)
void rgi_sg_make(const float a[3], const float d[3], float s, float out[7])
{
        put_sg(out, gi::SG{ v3(a), v3(d), s });
}
}
