// Exponential moving average (EMA) of the flat parameter vector, and the exchange of that average with the live weights.
//
// Not in the reference (its validation, checkpoints and decoding use the raw iterate).  las_ema_update moves the average one
// step towards the weights -- ema = decay*ema + (1 - decay)*p, two fp32 products and one fp32 sum in that order, (1 - decay)
// formed once on the host side of the launch; the build keeps -ffp-contract=off, so the result is defined bit for bit -- or,
// with init, copies the weights into an average that has never been written (ema is then not read at all).  las_ema_swap
// exchanges p and ema bit for bit and rewrites the bf16 shadow from the new p; it is its own inverse.
// Both are launches of their own behind the optimiser's: optim.hip does not know the average exists.
// HBM-bound by the byte count: update reads ema, p and writes ema = 12 B per element (init: reads p, writes ema = 8 B),
// swap reads p, ema and writes p, ema, p16 = 18 B per element (16 B without a shadow).
//
// Shape: 256 lanes, one float4 group per lane and stream, 64-bit element indices, ONE group per lane -- the grid covers the
// n >> 2 whole groups and is not capped.  A grid of 2048 blocks striding over the vector (the shape of optim.hip, and of
// noise.hip per range) was measured first and runs the 1 GiB c5 vector at 0.73 / 0.83 / 0.76 of 6.3 TB/s (update / init /
// swap) against 0.88 / 0.98 / 0.92 for this one; every cap in between lies in between, and more groups per lane and round
// do not make up for it.  The n & 3 elements behind the last whole group go one per lane of block 0.
// Nothing at an index >= n is read or written.
#include "las_common.h"

namespace {

template <bool INIT>
__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p, long n, float decay,
                                                         float rest) {
    const long n4 = n >> 2, g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g < n4) {
        const long i = g << 2;
        float4 v = ldg4(p + i);
        if (!INIT) {
            const float4 e = ldg4(ema + i);
            v = make_float4(decay * e.x + rest * v.x, decay * e.y + rest * v.y, decay * e.z + rest * v.z, decay * e.w + rest * v.w);
        }
        *(float4*)(ema + i) = v;
    }
    const long j = (n4 << 2) + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 3 && j < n) ema[j] = INIT ? p[j] : decay * ema[j] + rest * p[j];
}

__global__ __launch_bounds__(256) void ema_swap_kernel(float* __restrict__ p, bf16_t* __restrict__ p16, float* __restrict__ ema, long n) {
    const long n4 = n >> 2, g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g < n4) {
        const long i = g << 2;
        const float4 v = ldg4(p + i), e = ldg4(ema + i);
        *(float4*)(p + i) = e;
        *(float4*)(ema + i) = v;
        if (p16) store4_ct(p16 + i, e.x, e.y, e.z, e.w);
    }
    const long j = (n4 << 2) + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 3 && j < n) {
        const float v = p[j], e = ema[j];
        p[j] = e;
        ema[j] = v;
        if (p16) p16[j] = f2bf(e);
    }
}

// one block per 256 float4 groups, at least one (it carries the tail of an n < 4); grid.x holds 2^31 - 1 blocks
constexpr int64_t N_MAX = ((int64_t)1 << 40);
unsigned grid_x(long n) { const long b = (n / 4 + 255) / 256; return (unsigned)(b < 1 ? 1 : b); }

}  // namespace

extern "C" int las_ema_update(float* ema, const float* p, int64_t n, float decay, int init, void* stream) {
    LAS_CHECK_ARG(ema && p && n > 0 && n <= N_MAX);
    LAS_CHECK_ARG(((((uintptr_t)ema) | ((uintptr_t)p)) & 15) == 0);
    LAS_CHECK_ARG(decay >= 0.f && decay < 1.f);               // (false for NaN; asked of an initialising call too)
    if (init) {
        hipLaunchKernelGGL(ema_update_kernel<true>, dim3(grid_x(n)), dim3(256), 0, (hipStream_t)stream, ema, p, (long)n, 0.f, 0.f);
    } else {
        hipLaunchKernelGGL(ema_update_kernel<false>, dim3(grid_x(n)), dim3(256), 0, (hipStream_t)stream, ema, p, (long)n, decay,
                           1.f - decay);
    }
    LAS_LAUNCH_OK();
    return LAS_OK;
}

extern "C" int las_ema_swap(float* p, void* p_bf16, float* ema, int64_t n, void* stream) {
    LAS_CHECK_ARG(p && ema && n > 0 && n <= N_MAX);
    LAS_CHECK_ARG(((((uintptr_t)p) | ((uintptr_t)p_bf16) | ((uintptr_t)ema)) & 15) == 0);
    hipLaunchKernelGGL(ema_swap_kernel, dim3(grid_x(n)), dim3(256), 0, (hipStream_t)stream, p, (bf16_t*)p_bf16, ema, (long)n);
    LAS_LAUNCH_OK();
    return LAS_OK;
}
