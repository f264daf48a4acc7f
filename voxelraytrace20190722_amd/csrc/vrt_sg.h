// vrt_sg.h -- the reference's spherical-Gaussian algebra (gi::SG::SG,
// SG::integral, gi::prod, gi::inner_prod; VRT/voxel_octree.cc:497-528) and
// the light a scene's probes send to a point, written once for the host
// calls (the C library's expf) and the gfx950 kernels (expf_model): every
// function takes its expf as a functor and performs the reference's float32
// operations in the reference's order, one rounding each (compile with
// -ffp-contract=off, as everything that includes vrt_math.h).
#pragma once

#include "vrt_internal.h"

namespace vrt {

struct SGv {
        f3 a, d;
        float s;
};

// a vrt_sg record (7 floats {a, d, s}) as it is: nothing is re-normalised
VRT_HD SGv sg_load(const float *g)
{
        return SGv{ mk3(g[0], g[1], g[2]), mk3(g[3], g[4], g[5]), g[6] };
}
VRT_HD void sg_store(float *g, const SGv &v)
{
        g[0] = v.a.x, g[1] = v.a.y, g[2] = v.a.z;
        g[3] = v.d.x, g[4] = v.d.y, g[5] = v.d.z;
        g[6] = v.s;
}
VRT_HD void f3_store(float *o, f3 v) { o[0] = v.x, o[1] = v.y, o[2] = v.z; }
VRT_HD f3 mul3(f3 a, f3 b) { return mk3(a.x * b.x, a.y * b.y, a.z * b.z); }
VRT_HD f3 div3(f3 a, float s) { return mk3(a.x / s, a.y / s, a.z / s); }

// `2 * jql::pi` / `2.0f * jql::pi`, formed first in both expressions that use
// it; jql::pi is the float (VRT/graphics_math.h:23), so the product is exact
constexpr float kSGTwoPi = 2.0f * 3.1415926535897932384626f;

// SG::SG(a, d, s): d normalised (VRT/voxel_octree.cc:497-502)
VRT_HD SGv sg_make(f3 a, f3 d, float s) { return SGv{ a, normalize(d), s }; }

// SG::integral (:509-513): tmp = 1.0f - exp(-2.0f * s), the float overload;
// 2 * pi * (a / s) * tmp from the left
template <class Exp> VRT_HD f3 sg_integral(const SGv &g, Exp ex)
{
        const float tmp = 1.0f - ex(-2.0f * g.s);
        return (div3(g.a, g.s) * kSGTwoPi) * tmp;
}

// lhs.s * lhs.d + rhs.s * rhs.d, the vector prod and inner_prod start from
VRT_HD f3 sg_um(const SGv &l, const SGv &r) { return l.d * l.s + r.d * r.s; }

// gi::prod (:514-521); the result goes through SG's constructor
template <class Exp> VRT_HD SGv sg_prod(const SGv &l, const SGv &r, Exp ex)
{
        const float lm = l.s + r.s;
        const f3 d = div3(sg_um(l, r), lm);
        const float dl = length(d);
        return sg_make(mul3(l.a, r.a) * ex(lm * (dl - 1)), d, lm * dl);
}

// gi::inner_prod (:522-528)
template <class Exp> VRT_HD f3 sg_inner_prod(const SGv &l, const SGv &r, Exp ex)
{
        const float uml = length(sg_um(l, r));
        const f3 expo = mul3(l.a * ex(uml - l.s - r.s), r.a);
        const float other = 1.0f - ex(-2.0f * uml);
        return div3((expo * kSGTwoPi) * other, uml);
}

// vrt_probe_irradiance for one element (include/vrt.h): the leaf of the
// point by gi::cone_trace's descent without its level limit (VRT/
// voxel_octree.cc:261-269; centre = (min + max) * .5f, AABB3D::center as
// k_lm_aux and the oracle compute it), then the mean over the leaf's probes
// of the sum over their 14 stored lobes of inner_prod(lobe, q).  isect: 6
// floats {hit_p, normal}.  Returns the leaf's probe count.
template <class Exp>
VRT_HD int32_t probe_irradiance_one(const NodeRec *__restrict__ nodes, const uint2 *__restrict__ pnode,
                                    const uint32_t *__restrict__ pref, const float *__restrict__ sgs,
                                    const float *__restrict__ isect, f3 lobe_a, float lobe_s, Exp ex, f3 *rgb)
{
        *rgb = mk3(0.f, 0.f, 0.f);
        const float p[3] = { isect[0], isect[1], isect[2] };
        NodeRec nr = nodes[0];
        for (int k = 0; k < 3; ++k)
                if (!(p[k] >= nr.bmin[k] && p[k] <= nr.bmax[k]))  // a NaN is outside
                        return 0;
        uint32_t i = 0;
        // a tree is at most VRT_MAX_DEPTH levels deep; the bound only keeps a
        // damaged one from looping
        for (int l = 0; l < 2 * VRT_MAX_DEPTH && !(nr.a & kLeafBit); ++l) {
                uint32_t c = 0;
                c += p[0] > (nr.bmin[0] + nr.bmax[0]) * .5f ? 4u : 0u;
                c += p[1] > (nr.bmin[1] + nr.bmax[1]) * .5f ? 2u : 0u;
                c += p[2] > (nr.bmin[2] + nr.bmax[2]) * .5f ? 1u : 0u;
                i = nr.a + c;
                nr = nodes[i];
        }
        if (!(nr.a & kLeafBit))
                return 0;
        const uint2 pn = pnode[i];  // a leaf's {first entry in pref, length}
        if (pn.y == 0)
                return 0;
        const SGv q = sg_make(lobe_a, mk3(isect[3], isect[4], isect[5]), lobe_s);
        f3 acc = mk3(0.f, 0.f, 0.f);
        for (uint32_t k = 0; k < pn.y; ++k) {
                const float *g = sgs + (size_t)pref[pn.x + k] * (7 * kProbeSGs);
                for (int j = 0; j < kProbeSGs; ++j)
                        acc = acc + sg_inner_prod(sg_load(g + 7 * j), q, ex);
        }
        *rgb = div3(acc, (float)pn.y);
        return (int32_t)pn.y;
}

// the kernels' expf: the model of the host's, flavour `fused`
struct ModelExp {
        bool fused;
        VRT_HD float operator()(float x) const { return expf_model(x, fused); }
};

// Kernel launchers (vrt_sg.hip); every array in device memory, n > 0
hipError_t launch_sg_integral(const float *sgs, int64_t n, int fused, float *rgb, hipStream_t st);
hipError_t launch_sg_prod(const float *lhs, const float *rhs, int64_t n, int fused, float *out, hipStream_t st);
hipError_t launch_sg_inner_prod(const float *lhs, const float *rhs, int64_t n, int fused, float *rgb, hipStream_t st);
// count may be nullptr
hipError_t launch_probe_irradiance(const NodeRec *nodes, const ProbeDev &pd, const float *sgs, const float *isects,
                                   int64_t n, const float lobe_a[3], float lobe_s, int fused, float *rgb,
                                   int32_t *count, hipStream_t st);

}  // namespace vrt
