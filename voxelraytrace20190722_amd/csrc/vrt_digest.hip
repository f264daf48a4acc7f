// vrt_digest.hip -- the digest of include/vrt.h ("scene digest") on the
// device: a 64-bit word per array that a vrt_multi handle compares between its
// ranks after an update (VRT_MULTI_UPDATE_VERIFY), so that replicas are known
// to agree from 80 bytes per rank instead of a copy of every array.
//
//   digest = sum_i mix(((i + 1) * 0x9E3779B97F4A7C15) ^ w_i)   (mod 2^64)
//
// over the array's 32-bit words w_i, i counted from its first word.  Integer
// addition commutes, so lanes, waves and blocks may sum in any order: each
// lane accumulates in 64 bits, a wave reduces by shuffles, and lane 0 adds the
// wave's sum to out[item] with one 64-bit atomic.  Integers only; no LDS.
#include "vrt_internal.h"

namespace vrt {

namespace {

constexpr int kDigestBlock = 256;   // threads per block
constexpr int kDigestBlocks = 256;  // blocks per item: one grid pass = 256 * 256 16-byte loads

__device__ __forceinline__ uint64_t digest_term(uint64_t i, uint32_t w)
{
        uint64_t z = ((i + 1) * 0x9E3779B97F4A7C15ull) ^ (uint64_t)w;
        z ^= z >> 30;
        z *= 0xBF58476D1CE4E5B9ull;
        z ^= z >> 27;
        z *= 0x94D049BB133111EBull;
        z ^= z >> 31;
        return z;
}

// Item blockIdx.y.  A base is only 4-byte aligned in general (the per-record
// boxes start at refs - nr * 24; a caller's slice), so the array is cut into
// the words before the first 16-byte boundary (at most 3), a body of 16-byte
// loads dealt grid-stride over the item's blocks, and the words behind the
// last whole load (at most 3); head and tail are block 0's first lanes'.
__global__ __launch_bounds__(kDigestBlock) void k_digest(DigestItems it, unsigned long long *__restrict__ out)
{
        const int item = blockIdx.y;
        const uint32_t *__restrict__ p = static_cast<const uint32_t *>(it.p[item]);
        const uint64_t W = (uint64_t)it.bytes[item] >> 2;
        if (W == 0)
                return;
        uint64_t head = ((16u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2;
        if (head > W)
                head = W;
        const uint64_t nv = (W - head) >> 2;           // whole 16-byte loads
        const uint64_t tail0 = head + 4 * nv;          // first tail word
        uint64_t acc = 0;
        if (blockIdx.x == 0) {
                const uint64_t t = threadIdx.x;
                if (t < head)
                        acc += digest_term(t, p[t]);
                if (t < W - tail0)
                        acc += digest_term(tail0 + t, p[tail0 + t]);
        }
        const uint4 *__restrict__ body = reinterpret_cast<const uint4 *>(p + head);
        for (uint64_t v = (uint64_t)blockIdx.x * kDigestBlock + threadIdx.x; v < nv;
             v += (uint64_t)gridDim.x * kDigestBlock) {
                const uint4 q = body[v];
                const uint64_t i = head + 4 * v;
                acc += digest_term(i, q.x);
                acc += digest_term(i + 1, q.y);
                acc += digest_term(i + 2, q.z);
                acc += digest_term(i + 3, q.w);
        }
        for (int d = warpSize / 2; d > 0; d >>= 1)
                acc += (uint64_t)__shfl_down((unsigned long long)acc, d);
        if ((threadIdx.x & (warpSize - 1)) == 0 && acc != 0)
                atomicAdd(&out[item], (unsigned long long)acc);
}

}  // namespace

int64_t digest_pass_words() { return (int64_t)kDigestBlocks * kDigestBlock * 4; }

hipError_t launch_digest(const DigestItems &it, uint64_t *out, hipStream_t st)
{
        if (it.n <= 0 || it.n > kDigestItems)
                return hipErrorInvalidValue;
        if (hipError_t e = hipMemsetAsync(out, 0, (size_t)it.n * sizeof(uint64_t), st))
                return e;
        hipLaunchKernelGGL(k_digest, dim3(kDigestBlocks, (unsigned)it.n), dim3(kDigestBlock), 0, st, it,
                           reinterpret_cast<unsigned long long *>(out));
        return hipGetLastError();
}

}  // namespace vrt
