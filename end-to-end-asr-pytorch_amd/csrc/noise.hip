// Gaussian weight noise (variational noise) over ranges of the flat parameter vector.
//
// Not in the reference (its step evaluates the gradient at the weights it updates).  las_weight_noise_apply stashes the clean
// weights and writes W + sigma*z into the fp32 vector and its bf16 shadow; las_weight_noise_restore puts the stash back, shadow
// included, before the optimiser updates the clean weights with the gradient taken at the noisy ones.
// z is a pure function of (seed, step, absolute flat index): Philox4x32-10 on the index's float4 group, Box-Muller on the four
// words (contract in include/las_hip.h).  Neither the grid nor the range table enters it, so a group that a range covers only
// partly draws the same four values and uses the ones inside the range.
// HBM-bound by the byte count: apply reads p and writes clean, p, p16 = 14 B per noised element, restore 10 B.
#include "las_common.h"

namespace {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

// Philox4x32-10 (Salmon et al., SC'11): c <- (hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1, lo(M0*c0)), key bumped
// between rounds.  Each 64-bit product is one v_mad_u64_u32.
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c.x, p1 = (uint64_t)PHILOX_M1 * c.z;
        c = make_uint4((uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0);
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    return c;
}

// ((x >> 9) + 0.5) * 2^-23: exact in fp32, in [2^-24, 1 - 2^-24], so the logarithm below is finite and |z| <= sqrt(48 ln 2)
__device__ __forceinline__ float unit_open(uint32_t x) { return ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f; }

// Box-Muller.  The angle is 2*pi*u: sincospif takes it in half turns, and 2*u is exact, so no rounded 2*pi*u enters.
__device__ __forceinline__ void box_muller(uint32_t xa, uint32_t xb, float& za, float& zb) {
    const float r = sqrtf(-2.f * logf(unit_open(xa)));
    float s, c;
    sincospif(2.f * unit_open(xb), &s, &c);
    za = r * c;
    zb = r * s;
}

__device__ __forceinline__ float4 noise4(long g, uint32_t step, uint32_t k0, uint32_t k1) {
    const uint4 x = philox4x32_10(make_uint4((uint32_t)g, (uint32_t)((uint64_t)g >> 32), step, 0u), k0, k1);
    float4 z;
    box_muller(x.x, x.y, z.x, z.y);
    box_muller(x.z, x.w, z.z, z.w);
    return z;
}

// blockIdx.y = range, blockIdx.x grid-strides over the range's float4 groups.  A group wholly inside the range moves as 16-byte
// (bf16: 8-byte) accesses; the at most two groups a range covers partly are handled element by element under the mask, so that
// nothing outside the range is read or written (two ranges may share a group).
template <bool APPLY>
__global__ __launch_bounds__(256) void weight_noise_kernel(float* __restrict__ p, bf16_t* __restrict__ p16, float* __restrict__ clean,
                                                           long n, const int64_t* __restrict__ ranges, float sigma, uint32_t k0,
                                                           uint32_t k1, uint32_t step) {
    long lo = 0, hi = n;
    if (ranges) { lo = ranges[2 * blockIdx.y]; hi = lo + ranges[2 * blockIdx.y + 1]; }
    if (lo < 0) lo = 0;                                   // (the host builds the table inside [0, n); never step outside anyway)
    if (hi > n) hi = n;
    if (lo >= hi) return;
    const long g_end = (hi + 3) >> 2;
    for (long g = (lo >> 2) + (long)blockIdx.x * 256 + threadIdx.x; g < g_end; g += (long)gridDim.x * 256) {
        const long i = g << 2;
        const bool full = i >= lo && i + 4 <= hi;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f), z = v;
        if (full) v = ldg4(APPLY ? p + i : clean + i);    // in flight under the ~200 VALU instructions of the draw
        if (APPLY) z = noise4(g, step, k0, k1);
        if (full) {
            float4 w = v;
            if (APPLY) {
                *(float4*)(clean + i) = v;
                w = make_float4(v.x + sigma * z.x, v.y + sigma * z.y, v.z + sigma * z.z, v.w + sigma * z.w);
            }
            *(float4*)(p + i) = w;
            if (p16) store4_ct(p16 + i, w.x, w.y, w.z, w.w);
        } else {
            const float zz[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long j = i + k;
                if (j >= lo && j < hi) {
                    float w;
                    if (APPLY) {
                        const float vj = p[j];
                        clean[j] = vj;
                        w = vj + sigma * zz[k];
                    } else {
                        w = clean[j];
                    }
                    p[j] = w;
                    if (p16) p16[j] = f2bf(w);
                }
            }
        }
    }
}

// grid.x covers the longest range (capped at 2048 blocks, grid-strided); the host passes the table on the device, so the longest
// range is not known here: n bounds it.
unsigned grid_x(long n) { long b = (n / 4 + 256) / 256; return (unsigned)(b > 2048 ? 2048 : (b < 1 ? 1 : b)); }

int check_args(const void* p, const void* p16, const void* clean, int64_t n, const int64_t* ranges, int R) {
    LAS_CHECK_ARG(p && clean && n > 0);
    LAS_CHECK_ARG(((((uintptr_t)p) | ((uintptr_t)p16) | ((uintptr_t)clean)) & 15) == 0);
    LAS_CHECK_ARG(ranges == nullptr || ((R > 0 && R <= 65535) && (((uintptr_t)ranges) & 7) == 0));
    return LAS_OK;
}

}  // namespace

extern "C" int las_weight_noise_apply(float* p, void* p_bf16, float* clean, int64_t n, const int64_t* ranges, int R, float sigma,
                                      uint64_t seed, uint32_t step, void* stream) {
    const int rc = check_args(p, p_bf16, clean, n, ranges, R);
    if (rc != LAS_OK) return rc;
    LAS_CHECK_ARG(sigma >= 0.f);                          // (false for NaN)
    hipLaunchKernelGGL(weight_noise_kernel<true>, dim3(grid_x(n), ranges ? R : 1), dim3(256), 0, (hipStream_t)stream, p,
                       (bf16_t*)p_bf16, clean, (long)n, ranges, sigma, (uint32_t)seed, (uint32_t)(seed >> 32), step);
    LAS_LAUNCH_OK();
    return LAS_OK;
}

extern "C" int las_weight_noise_restore(float* p, void* p_bf16, const float* clean, int64_t n, const int64_t* ranges, int R,
                                        void* stream) {
    const int rc = check_args(p, p_bf16, clean, n, ranges, R);
    if (rc != LAS_OK) return rc;
    hipLaunchKernelGGL(weight_noise_kernel<false>, dim3(grid_x(n), ranges ? R : 1), dim3(256), 0, (hipStream_t)stream, p,
                       (bf16_t*)p_bf16, (float*)clean, (long)n, ranges, 0.f, 0u, 0u, 0u);
    LAS_LAUNCH_OK();
    return LAS_OK;
}
