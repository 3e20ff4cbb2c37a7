// Attention cross-entropy with per-utterance normalisation, and the scalar reductions of the joint loss.
//
// Replaces CrossEntropyLoss(ignore_index=0, reduction='none') + sum_t / sum(y!=0) + batch mean at reference
// src/solver.py:90,149-155, and the 'mean' reduction of CTCLoss (nll_b / clamp(target_len_b, 1), batch mean,
// solver.py:93,160).  One pass over the logits computes the row log-sum-exp, the row loss and writes the
// gradient row; the reductions are deterministic (no float atomics).
#include "las_common.h"

namespace {

// one block per (b,t) row of logits [B][L][V]; label = y[b][t+1]
__global__ __launch_bounds__(256) void ce_rows_kernel(const float* __restrict__ logits, const long long* __restrict__ y,
                                                      int Ly, const int32_t* __restrict__ ntok, int B, int L, int V,
                                                      float gscale, float* __restrict__ rowloss,
                                                      float* __restrict__ dlogits) {
    __shared__ float red[32];
    const int row = blockIdx.x, b = row / L, t = row % L;
    const int label = (int)y[(long)b * Ly + t + 1];
    const float* x = logits + (long)row * V;
    float* g = dlogits ? dlogits + (long)row * V : nullptr;
    if (label == 0 || label >= V || label < 0) {            // ignore_index = 0
        if (threadIdx.x == 0) rowloss[row] = 0.f;
        if (g) for (int i = threadIdx.x; i < V; i += 256) g[i] = 0.f;
        return;
    }
    float m = -INFINITY;
    for (int i = threadIdx.x; i < V; i += 256) m = fmaxf(m, x[i]);
    m = block_max(m, red);
    float s = 0.f;
    for (int i = threadIdx.x; i < V; i += 256) s += expf(x[i] - m);
    s = block_sum(s, red);
    const float lse = m + logf(s);
    if (threadIdx.x == 0) rowloss[row] = lse - x[label];
    if (g) {
        const float w = gscale / ((float)B * (float)max(ntok[b], 1));
        for (int i = threadIdx.x; i < V; i += 256) g[i] = w * (expf(x[i] - lse) - (i == label ? 1.f : 0.f));
    }
}

// ---- label smoothing: target t_v = (1-eps)*[v == label] + eps*q_v, q = prior [V] or 1/V (F.cross_entropy(label_smoothing=eps)
// is the uniform case).  rowloss = lse - (1-eps)*x[label] - eps*sum_v q_v x_v;  g_v = w*(softmax_v - t_v).
//
// V <= 64*E: one wave per (b,t) row, four rows per workgroup.  Lane i holds elements i, i+64, ... (coalesced) in registers, so
// the row is read once; the three reductions are DPP wave reductions: no LDS, no barrier.  Everything that decides control
// flow (row, label) is wave-uniform, so the reductions always run with all 64 lanes active.
template <int E>
__global__ __launch_bounds__(256) void ce_ls_wave_kernel(const float* __restrict__ logits, const long long* __restrict__ y,
                                                         int Ly, const int32_t* __restrict__ ntok, int B, int L, int V,
                                                         float gscale, float eps, const float* __restrict__ prior,
                                                         float* __restrict__ rowloss, float* __restrict__ dlogits) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)B * L) return;                             // (whole wave)
    const int b = (int)(row / L), t = (int)(row % L);
    const int label = (int)y[(long)b * Ly + t + 1];
    const float* x = logits + row * V;
    float* g = dlogits ? dlogits + row * V : nullptr;
    if (label == 0 || label >= V || label < 0) {            // ignore_index = 0
        if (lane == 0) rowloss[row] = 0.f;
        if (g) {
#pragma unroll
            for (int e = 0; e < E; ++e)
                if (lane + 64 * e < V) g[lane + 64 * e] = 0.f;
        }
        return;
    }
    // unconditional loads from clamped indices, masked on the data (las_common.h, ldg4)
    float xv[E], qv[E];
    const float qu = 1.f / (float)V;
#pragma unroll
    for (int e = 0; e < E; ++e) xv[e] = x[min(lane + 64 * e, V - 1)];
    if (prior) {
#pragma unroll
        for (int e = 0; e < E; ++e) qv[e] = prior[min(lane + 64 * e, V - 1)];
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) qv[e] = qu;
    }
    float m = -INFINITY, dot = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const bool ok = lane + 64 * e < V;
        dot += ok ? qv[e] * xv[e] : 0.f;
        xv[e] = ok ? xv[e] : -INFINITY;
        qv[e] = ok ? qv[e] : 0.f;
        m = fmaxf(m, xv[e]);
    }
    m = wave_max(m);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) s += expf(xv[e] - m);       // (padding: expf(-inf) = 0)
    s = wave_sum(s);
    dot = wave_sum(dot);
    const float lse = m + logf(s);
    const float conf = 1.f - eps;
    if (lane == 0) rowloss[row] = lse - conf * x[label] - eps * dot;
    if (g) {
        const float w = gscale / ((float)B * (float)max(ntok[b], 1));
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = lane + 64 * e;
            if (i < V) g[i] = w * (expf(xv[e] - lse) - ((i == label ? conf : 0.f) + eps * qv[e]));
        }
    }
}

// V > 1024: one workgroup per row.  A thread's share of a row is units of W consecutive floats, unit u = tid + 256*k: W = 4
// (one 16-byte load / store per unit) when V % 4 == 0 and every base is 16-byte aligned, else W = 1.  Eight values per thread
// are requested before the first is used (unconditional loads from clamped units, masked on the data: las_common.h, ldg4).
template <int W>
__device__ __forceinline__ void ce_ld8(const float* __restrict__ p, int u0, int NU, float (&v)[8]) {
#pragma unroll
    for (int k = 0; k < 8 / W; ++k) {
        const long u = min(u0 + 256 * k, NU - 1);
        if constexpr (W == 4) {
            const float4 t = ldg4(p + 4 * u);
            v[4 * k] = t.x; v[4 * k + 1] = t.y; v[4 * k + 2] = t.z; v[4 * k + 3] = t.w;
        } else {
            v[k] = p[u];
        }
    }
}
// Pass 1 keeps a running maximum and a rescaled sum per thread (online softmax), one rescale per group of eight values, and
// the q.x dot in the same sweep; pass 2 reads the row again (a cache hit) for the gradient.
template <int W>
__global__ __launch_bounds__(256) void ce_ls_block_kernel(const float* __restrict__ logits, const long long* __restrict__ y,
                                                          int Ly, const int32_t* __restrict__ ntok, int B, int L, int V,
                                                          float gscale, float eps, const float* __restrict__ prior,
                                                          float* __restrict__ rowloss, float* __restrict__ dlogits) {
    __shared__ float red[32];
    const int row = blockIdx.x, b = row / L, t = row % L;
    const int label = (int)y[(long)b * Ly + t + 1];
    const float* x = logits + (long)row * V;
    float* g = dlogits ? dlogits + (long)row * V : nullptr;
    if (label == 0 || label >= V || label < 0) {            // ignore_index = 0
        if (threadIdx.x == 0) rowloss[row] = 0.f;
        if (g) for (int i = threadIdx.x; i < V; i += 256) g[i] = 0.f;
        return;
    }
    const int NU = V / W;                                    // (W = 4 only when V % 4 == 0)
    const float qu = 1.f / (float)V;
    float xv[8], qv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) qv[j] = qu;
    float m = -INFINITY, s = 0.f, dot = 0.f;
    for (int u0 = threadIdx.x; u0 < NU; u0 += 256 * (8 / W)) {
        ce_ld8<W>(x, u0, NU, xv);
        if (prior) ce_ld8<W>(prior, u0, NU, qv);
        float gm = -INFINITY;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool ok = u0 + 256 * (j / W) < NU;
            dot += ok ? qv[j] * xv[j] : 0.f;
            xv[j] = ok ? xv[j] : -INFINITY;
            gm = fmaxf(gm, xv[j]);
        }
        const float mn = fmaxf(m, gm);
        if (mn > -INFINITY) {                                // (a group of -inf logits adds nothing)
            float a = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) a += expf(xv[j] - mn);
            s = s * expf(m - mn) + a;                        // (first group: s = 0 * expf(-inf))
            m = mn;
        }
    }
    const float bm = block_max(m, red);
    s = block_sum(m > -INFINITY ? s * expf(m - bm) : 0.f, red);
    dot = block_sum(dot, red);
    const float lse = bm + logf(s);
    const float conf = 1.f - eps;
    if (threadIdx.x == 0) rowloss[row] = lse - conf * x[label] - eps * dot;
    if (g) {
        const float w = gscale / ((float)B * (float)max(ntok[b], 1));
        for (int u0 = threadIdx.x; u0 < NU; u0 += 256 * (8 / W)) {
            ce_ld8<W>(x, u0, NU, xv);
            if (prior) ce_ld8<W>(prior, u0, NU, qv);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int i = (u0 + 256 * (j / W)) * W + j % W;
                xv[j] = w * (expf(xv[j] - lse) - ((i == label ? conf : 0.f) + eps * qv[j]));
            }
#pragma unroll
            for (int k = 0; k < 8 / W; ++k) {
                const int u = u0 + 256 * k;
                if (u < NU) {
                    if constexpr (W == 4)
                        *reinterpret_cast<float4*>(__builtin_assume_aligned(g + 4 * (long)u, 16)) =
                            make_float4(xv[4 * k], xv[4 * k + 1], xv[4 * k + 2], xv[4 * k + 3]);
                    else
                        g[u] = xv[k];
                }
            }
        }
    }
}

// loss = mean_b( sum_t rowloss[b,t] / max(ntok_b,1) );  one block
__global__ __launch_bounds__(256) void ce_finish_kernel(const float* __restrict__ rowloss,
                                                        const int32_t* __restrict__ ntok, int B, int L,
                                                        float* __restrict__ loss) {
    __shared__ float red[32];
    float acc = 0.f;
    for (int b = 0; b < B; ++b) {
        float s = 0.f;
        for (int t = threadIdx.x; t < L; t += 256) s += rowloss[(long)b * L + t];
        s = block_sum(s, red);
        acc += s / (float)max(ntok[b], 1);
    }
    if (threadIdx.x == 0) loss[0] = acc / (float)B;
}

// out = mean_b x[b] / max(n[b],1)
__global__ void norm_mean_fwd_kernel(const float* __restrict__ x, const int32_t* __restrict__ n, int B,
                                     float* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc += x[b] / (float)max(n[b], 1);
        out[0] = acc / (float)B;
    }
}
// gx[b] = g * scale / (B * max(n[b],1))
__global__ void norm_mean_bwd_kernel(const float* __restrict__ g, float scale, const int32_t* __restrict__ n, int B,
                                     float* __restrict__ gx) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) gx[b] = g[0] * scale / ((float)B * (float)max(n[b], 1));
}

// x *= alpha[0] (device scalar)
__global__ __launch_bounds__(256) void scale_kernel(float* __restrict__ x, long n, const float* __restrict__ alpha) {
    const float a = alpha[0];
    if (a == 1.f) return;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) x[i] *= a;
}

// out[0] = wa*a[0] + wb*b[0]   (either pointer may be NULL)
__global__ void combine_kernel(const float* a, float wa, const float* b, float wb, float* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = (a ? wa * a[0] : 0.f) + (b ? wb * b[0] : 0.f);
}


// pred[row] = argmax_v logits[row][v] (first maximum)
__global__ __launch_bounds__(256) void argmax_rows_kernel(const float* __restrict__ logits, int V, int32_t* __restrict__ pred) {
    __shared__ float bv[256];
    __shared__ int bi[256];
    const float* x = logits + (long)blockIdx.x * V;
    float v = -INFINITY; int idx = 0;
    for (int i = threadIdx.x; i < V; i += 256) if (x[i] > v) { v = x[i]; idx = i; }
    bv[threadIdx.x] = v; bi[threadIdx.x] = idx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            const float ov = bv[threadIdx.x + o]; const int oi = bi[threadIdx.x + o];
            if (ov > bv[threadIdx.x] || (ov == bv[threadIdx.x] && oi < bi[threadIdx.x])) { bv[threadIdx.x] = ov; bi[threadIdx.x] = oi; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) pred[blockIdx.x] = bi[0];
}

// mean over utterances of token accuracy up to the first 0 label (reference postprocess.py:121-133)
__global__ void token_acc_kernel(const int32_t* __restrict__ pred, const long long* __restrict__ y, int Ly, int B, int L,
                                 float* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float acc = 0.f;
    for (int b = 0; b < B; ++b) {
        int correct = 0, total = 0;
        for (int t = 0; t < L; ++t) {
            const long long l = y[(long)b * Ly + t + 1];
            if (l == 0) break;
            correct += (pred[(long)b * L + t] == (int)l);
            ++total;
        }
        acc += (float)correct / (float)max(total, 1);
    }
    out[0] = acc / (float)B;
}

}  // namespace

extern "C" int las_ce_loss(const float* logits, const int64_t* y, int Ly, const int32_t* ntok, int B, int L, int V,
                           float gscale, float* rowloss, float* loss, float* dlogits, void* stream) {
    LAS_CHECK_ARG(logits && y && ntok && rowloss && loss && B > 0 && L > 0 && V > 1 && Ly >= L + 1);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ce_rows_kernel, dim3(B * L), dim3(256), 0, st, logits, (const long long*)y, Ly, ntok, B, L, V, gscale,
                       rowloss, dlogits);
    LAS_LAUNCH_OK();
    hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(256), 0, st, rowloss, ntok, B, L, loss);
    LAS_LAUNCH_OK();
    return LAS_OK;
}

extern "C" int las_ce_loss_ls(const float* logits, const int64_t* y, int Ly, const int32_t* ntok, int B, int L, int V,
                              float gscale, float eps, const float* prior, float* rowloss, float* loss, float* dlogits,
                              void* stream) {
    LAS_CHECK_ARG(logits && y && ntok && rowloss && loss && B > 0 && L > 0 && V > 1 && Ly >= L + 1);
    LAS_CHECK_ARG(eps >= 0.f && eps < 1.f);                 // (NaN fails both)
    hipStream_t st = (hipStream_t)stream;
    const long long* yl = (const long long*)y;
    const dim3 wgrid((unsigned)(((long)B * L + 3) / 4)), blk(256);
    if (V <= 64)
        hipLaunchKernelGGL(ce_ls_wave_kernel<1>, wgrid, blk, 0, st, logits, yl, Ly, ntok, B, L, V, gscale, eps, prior, rowloss, dlogits);
    else if (V <= 256)
        hipLaunchKernelGGL(ce_ls_wave_kernel<4>, wgrid, blk, 0, st, logits, yl, Ly, ntok, B, L, V, gscale, eps, prior, rowloss, dlogits);
    else if (V <= 1024)
        hipLaunchKernelGGL(ce_ls_wave_kernel<16>, wgrid, blk, 0, st, logits, yl, Ly, ntok, B, L, V, gscale, eps, prior, rowloss, dlogits);
    else if (V % 4 == 0 && ((uintptr_t)logits | (uintptr_t)dlogits | (uintptr_t)prior) % 16 == 0)
        hipLaunchKernelGGL(ce_ls_block_kernel<4>, dim3(B * L), blk, 0, st, logits, yl, Ly, ntok, B, L, V, gscale, eps, prior, rowloss, dlogits);
    else
        hipLaunchKernelGGL(ce_ls_block_kernel<1>, dim3(B * L), blk, 0, st, logits, yl, Ly, ntok, B, L, V, gscale, eps, prior, rowloss, dlogits);
    LAS_LAUNCH_OK();
    hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(256), 0, st, rowloss, ntok, B, L, loss);
    LAS_LAUNCH_OK();
    return LAS_OK;
}

extern "C" int las_norm_mean_fwd(const float* x, const int32_t* n, int B, float* out, void* stream) {
    LAS_CHECK_ARG(x && n && out && B > 0);
    hipLaunchKernelGGL(norm_mean_fwd_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, x, n, B, out);
    LAS_LAUNCH_OK();
    return LAS_OK;
}

extern "C" int las_norm_mean_bwd(const float* g, float scale, const int32_t* n, int B, float* gx, void* stream) {
    LAS_CHECK_ARG(g && n && gx && B > 0);
    hipLaunchKernelGGL(norm_mean_bwd_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, g, scale, n, B, gx);
    LAS_LAUNCH_OK();
    return LAS_OK;
}

extern "C" int las_scale_dev(float* x, int64_t n, const float* alpha, void* stream) {
    LAS_CHECK_ARG(x && alpha && n >= 0);
    if (n == 0) return LAS_OK;
    long blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(scale_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, (long)n, alpha);
    LAS_LAUNCH_OK();
    return LAS_OK;
}

extern "C" int las_combine2(const float* a, float wa, const float* b, float wb, float* out, void* stream) {
    LAS_CHECK_ARG(out && (a || b));
    hipLaunchKernelGGL(combine_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a, wa, b, wb, out);
    LAS_LAUNCH_OK();
    return LAS_OK;
}

extern "C" int las_argmax_rows(const float* logits, int rows, int V, int32_t* pred, void* stream) {
    LAS_CHECK_ARG(logits && pred && rows > 0 && V > 0);
    hipLaunchKernelGGL(argmax_rows_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, logits, V, pred);
    LAS_LAUNCH_OK();
    return LAS_OK;
}

extern "C" int las_token_acc(const int32_t* pred, const int64_t* y, int Ly, int B, int L, float* out, void* stream) {
    LAS_CHECK_ARG(pred && y && out && B > 0 && L > 0 && Ly >= L + 1);
    hipLaunchKernelGGL(token_acc_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, pred, (const long long*)y, Ly, B, L, out);
    LAS_LAUNCH_OK();
    return LAS_OK;
}
