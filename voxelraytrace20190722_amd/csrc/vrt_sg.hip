// vrt_sg.hip -- the SG algebra and the probes' irradiance on the device
// (vrt_sg_integral_device, vrt_sg_prod_device, vrt_sg_inner_prod_device,
// vrt_probe_irradiance_device).  One lane per element in grid-stride, 256
// threads per block; the float operations are vrt_sg.h's, shared with the
// host calls, with the host expf's bits from expf_model (fused: the detected
// flavour, uniform over the launch).  The 28-byte records are read as
// scalars: a wave's 64 records are 1792 contiguous bytes, so every line
// fetched is used whole.  Timings: DESIGN.md 4.5.
#include <algorithm>

#include "vrt_sg.h"

namespace vrt {

namespace {

constexpr int kSGBlock = 256;
// blocks of a launch: enough for 8 per CU, grid-stride beyond
constexpr int64_t kSGMaxBlocks = 2048;

__global__ __launch_bounds__(kSGBlock) void k_sg_integral(const float *__restrict__ sgs, int64_t n, int fused,
                                                           float *__restrict__ rgb)
{
        const ModelExp ex{ fused != 0 };
        for (int64_t i = (int64_t)blockIdx.x * kSGBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSGBlock)
                f3_store(rgb + 3 * i, sg_integral(sg_load(sgs + 7 * i), ex));
}

__global__ __launch_bounds__(kSGBlock) void k_sg_prod(const float *__restrict__ lhs, const float *__restrict__ rhs,
                                                       int64_t n, int fused, float *__restrict__ out)
{
        const ModelExp ex{ fused != 0 };
        for (int64_t i = (int64_t)blockIdx.x * kSGBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSGBlock)
                sg_store(out + 7 * i, sg_prod(sg_load(lhs + 7 * i), sg_load(rhs + 7 * i), ex));
}

__global__ __launch_bounds__(kSGBlock) void k_sg_inner_prod(const float *__restrict__ lhs,
                                                             const float *__restrict__ rhs, int64_t n, int fused,
                                                             float *__restrict__ rgb)
{
        const ModelExp ex{ fused != 0 };
        for (int64_t i = (int64_t)blockIdx.x * kSGBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSGBlock)
                f3_store(rgb + 3 * i, sg_inner_prod(sg_load(lhs + 7 * i), sg_load(rhs + 7 * i), ex));
}

// One lane per point: at most max_depth dependent node reads down to the
// leaf (nearby points share the upper levels' lines), then the leaf's probe
// list.  Lanes whose leaf holds no probe write +0 and wait for the others.
__global__ __launch_bounds__(kSGBlock) void k_probe_irradiance(const NodeRec *__restrict__ nodes,
                                                                const uint2 *__restrict__ pnode,
                                                                const uint32_t *__restrict__ pref,
                                                                const float *__restrict__ sgs,
                                                                const float *__restrict__ isects, int64_t n, float ax,
                                                                float ay, float az, float ls, int fused,
                                                                float *__restrict__ rgb, int32_t *__restrict__ count)
{
        const ModelExp ex{ fused != 0 };
        for (int64_t i = (int64_t)blockIdx.x * kSGBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSGBlock) {
                f3 c;
                const int32_t k = probe_irradiance_one(nodes, pnode, pref, sgs, isects + 6 * i, mk3(ax, ay, az), ls, ex,
                                                       &c);
                f3_store(rgb + 3 * i, c);
                if (count)
                        count[i] = k;
        }
}

unsigned sg_grid(int64_t n) { return (unsigned)std::min<int64_t>((n + kSGBlock - 1) / kSGBlock, kSGMaxBlocks); }

}  // namespace

hipError_t launch_sg_integral(const float *sgs, int64_t n, int fused, float *rgb, hipStream_t st)
{
        if (n <= 0)
                return hipSuccess;
        hipLaunchKernelGGL(k_sg_integral, dim3(sg_grid(n)), dim3(kSGBlock), 0, st, sgs, n, fused, rgb);
        return hipGetLastError();
}

hipError_t launch_sg_prod(const float *lhs, const float *rhs, int64_t n, int fused, float *out, hipStream_t st)
{
        if (n <= 0)
                return hipSuccess;
        hipLaunchKernelGGL(k_sg_prod, dim3(sg_grid(n)), dim3(kSGBlock), 0, st, lhs, rhs, n, fused, out);
        return hipGetLastError();
}

hipError_t launch_sg_inner_prod(const float *lhs, const float *rhs, int64_t n, int fused, float *rgb, hipStream_t st)
{
        if (n <= 0)
                return hipSuccess;
        hipLaunchKernelGGL(k_sg_inner_prod, dim3(sg_grid(n)), dim3(kSGBlock), 0, st, lhs, rhs, n, fused, rgb);
        return hipGetLastError();
}

hipError_t launch_probe_irradiance(const NodeRec *nodes, const ProbeDev &pd, const float *sgs, const float *isects,
                                   int64_t n, const float lobe_a[3], float lobe_s, int fused, float *rgb,
                                   int32_t *count, hipStream_t st)
{
        if (n <= 0)
                return hipSuccess;
        hipLaunchKernelGGL(k_probe_irradiance, dim3(sg_grid(n)), dim3(kSGBlock), 0, st, nodes, pd.pnode, pd.pref, sgs,
                           isects, n, lobe_a[0], lobe_a[1], lobe_a[2], lobe_s, fused, rgb, count);
        return hipGetLastError();
}

}  // namespace vrt
