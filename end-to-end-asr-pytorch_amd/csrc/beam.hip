// Device side of the joint CTC/attention beam search (reference src/asr.py:155-258, src/ctc.py): per-row
// log-softmax and top-k over the vocabulary, the CTC prefix scorer batched over (hypothesis, candidate) pairs, and the
// score combination.  The reference walks T' frames in numpy once per hypothesis and candidate on the host; here one
// thread owns one (hypothesis, candidate) lattice column pair and all beam x candidates pairs advance together.
#include "las_common.h"

namespace {

constexpr float LOGZERO = -100000000.0f;            // ctc.py:11

// float32 logaddexp as numpy's npy_logaddexpf (max + log1p(exp(-|d|))), on the hardware exp2/log2 units: the T'-long
// chain of a (hypothesis, candidate) pair is three of these per frame, strictly sequential, so their latency IS the
// kernel time.  log(1 + e) instead of log1p(e) differs by < 6e-8 absolute (e < 1), far below the float32 resolution of
// the log-probabilities being summed.
__device__ __forceinline__ float logaddexp_np(float x, float y) {
    const float m = fmaxf(x, y), d = -fabsf(x - y);
    return m + __logf(1.f + __expf(d));
}

__global__ __launch_bounds__(256) void log_softmax_rows_kernel(const float* __restrict__ x, int V, float* __restrict__ out) {
    __shared__ float red[32];
    const float* p = x + (long)blockIdx.x * V;
    float* o = out + (long)blockIdx.x * V;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < V; i += 256) m = fmaxf(m, p[i]);
    m = block_max(m, red);
    float s = 0.f;
    for (int i = threadIdx.x; i < V; i += 256) s += expf(p[i] - m);
    s = block_sum(s, red);
    const float lse = m + logf(s);
    for (int i = threadIdx.x; i < V; i += 256) o[i] = p[i] - lse;
}

// k largest of each row, descending, ties to the lower index; one workgroup per row, the row staged in LDS
__global__ __launch_bounds__(256) void topk_rows_kernel(const float* __restrict__ x, int V, int k,
                                                        float* __restrict__ vals, int32_t* __restrict__ idx) {
    extern __shared__ float row[];
    __shared__ float bv[256];
    __shared__ int bi[256];
    const float* p = x + (long)blockIdx.x * V;
    for (int i = threadIdx.x; i < V; i += 256) row[i] = p[i];
    __syncthreads();
    for (int j = 0; j < k; ++j) {
        float v = -INFINITY;
        int ix = V;
        for (int i = threadIdx.x; i < V; i += 256) {
            const float r = row[i];
            if (r > v || (r == v && i < ix) || (ix == V && r != r)) { v = r; ix = i; }
        }
        bv[threadIdx.x] = v; bi[threadIdx.x] = ix;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (threadIdx.x < o) {
                const float ov = bv[threadIdx.x + o]; const int oi = bi[threadIdx.x + o];
                if (ov > bv[threadIdx.x] || (ov == bv[threadIdx.x] && oi < bi[threadIdx.x])) { bv[threadIdx.x] = ov; bi[threadIdx.x] = oi; }
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const int w = min(bi[0], V - 1);
            vals[(long)blockIdx.x * k + j] = bv[0];
            idx[(long)blockIdx.x * k + j] = w;
            row[w] = -INFINITY;
        }
        __syncthreads();
    }
}

// r0[t] = {LOGZERO, sum_{u<=t} lp[u][blank]}   (CTCPrefixScore.init_state, ctc.py:19-27)
__global__ void ctc_prefix_init_kernel(const float* __restrict__ lp, int T, int V, float* __restrict__ r0) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float acc = 0.f;
    for (int t = 0; t < T; ++t) {
        acc = t == 0 ? lp[0] : acc + lp[(long)t * V];
        r0[2 * t] = LOGZERO;
        r0[2 * t + 1] = acc;
    }
}

// CTCPrefixScore.cheap_compute (ctc.py:65-101) of one (hypothesis, candidate c) pair over the T frames of lp: rp [T][2] the
// prefix's state, ro [T][2] the extended prefix's; returns psi.  len / lc: prefix length and last token (0 when empty).
__device__ __forceinline__ float ctc_prefix_pair(const float* __restrict__ lp, int T, int V, const float* __restrict__ rp,
                                                 float* __restrict__ ro, int c, int len, int lc) {
    const int start = max(1, len);
    for (int t = 0; t < min(start, T); ++t) { ro[2 * t] = LOGZERO; ro[2 * t + 1] = LOGZERO; }
    float rn = LOGZERO, rb = LOGZERO;                // r[start-1][0], r[start-1][1]
    if (len == 0) { rn = lp[c]; ro[0] = rn; }        // empty prefix: r[0][0] = x[0][c]  (start = 1)
    float p = rn;                                    // psi = r[start-1][0]
    // the operands of the recurrence (r_prev, lp) do not depend on it: 8 frames are requested together, then consumed
    constexpr int U = 8;
    for (int t0 = start; t0 < T; t0 += U) {
        float2 rv[U];
        float xc[U], xb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = min(t0 + u, T - 1);
            rv[u] = *(const float2*)(rp + 2 * (t - 1));
            xc[u] = lp[(long)t * V + c];
            xb[u] = lp[(long)t * V];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = t0 + u;
            if (t < T) {
                const float pb = c == lc ? LOGZERO : rv[u].y;
                const float phi = logaddexp_np(rv[u].x, pb);
                const float nn = logaddexp_np(rn, phi) + xc[u];
                const float nb = logaddexp_np(rb, rn) + xb[u];
                p = logaddexp_np(p, phi + xc[u]);
                rn = nn; rb = nb;
                *(float2*)(ro + 2 * t) = make_float2(nn, nb);
            }
        }
    }
    return p;
}

// thread = (hypothesis n, candidate j) pair
__global__ __launch_bounds__(64) void ctc_prefix_score_kernel(const float* __restrict__ lp, int T, int V,
                                                              const float* __restrict__ r_prev, const int32_t* __restrict__ last,
                                                              const int32_t* __restrict__ plen, const int32_t* __restrict__ cand,
                                                              int N, int K, float* __restrict__ psi, float* __restrict__ r_out) {
    const int pair = blockIdx.x * 64 + threadIdx.x;
    if (pair >= N * K) return;
    const int n = pair / K;
    const int c = min(max(cand[pair], 0), V - 1);
    const int len = plen[n], lc = len > 0 ? last[n] : 0;
    psi[pair] = ctc_prefix_pair(lp, T, V, r_prev + (long)n * T * 2, r_out + (long)pair * T * 2, c, len, lc);
}

// the same over several utterances: lp [U][Tmax][V], states laid out on Tmax, row n belongs to utterance row_utt[n] and
// walks that utterance's T_u frames only
__global__ __launch_bounds__(64) void ctc_prefix_score_batch_kernel(const float* __restrict__ lp, int Tmax, int V, int U,
                                                                    const int32_t* __restrict__ T_u, const int32_t* __restrict__ row_utt,
                                                                    const float* __restrict__ r_prev, const int32_t* __restrict__ last,
                                                                    const int32_t* __restrict__ plen, const int32_t* __restrict__ cand,
                                                                    int N, int K, float* __restrict__ psi, float* __restrict__ r_out) {
    const int pair = blockIdx.x * 64 + threadIdx.x;
    if (pair >= N * K) return;
    const int n = pair / K;
    const int u = min(max(row_utt[n], 0), U - 1);
    const int T = min(max(T_u[u], 1), Tmax);
    const int c = min(max(cand[pair], 0), V - 1);
    const int len = max(plen[n], 0), lc = len > 0 ? last[n] : 0;
    psi[pair] = ctc_prefix_pair(lp + (long)u * Tmax * V, T, V, r_prev + (long)n * Tmax * 2, r_out + (long)pair * Tmax * 2, c, len, lc);
}

__global__ void ctc_prefix_init_batch_kernel(const float* __restrict__ lp, int U, int Tmax, int V, const int32_t* __restrict__ T_u,
                                             float* __restrict__ r0) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= U) return;
    const int T = min(max(T_u[u], 1), Tmax);
    const float* x = lp + (long)u * Tmax * V;
    float* r = r0 + (long)u * Tmax * 2;
    float acc = 0.f;
    for (int t = 0; t < T; ++t) {
        acc = t == 0 ? x[0] : acc + x[(long)t * V];
        r[2 * t] = LOGZERO;
        r[2 * t + 1] = acc;
    }
}

// cur[n][:] = (1-lam)*cur + lam*hack, hack = -1e6 except hack[cand[j]] = psi[n][j] - prev_ctc[n]; then cur[n][0] = -1e7
// (asr.py:218-229)
__global__ __launch_bounds__(256) void beam_combine_kernel(float* __restrict__ cur, int V, const int32_t* __restrict__ cand,
                                                           const float* __restrict__ psi, const float* __restrict__ prev_ctc,
                                                           int K, float lam) {
    extern __shared__ float co[];                    // [K] attention log-probs of the candidates
    const int n = blockIdx.x;
    float* row = cur + (long)n * V;
    for (int j = threadIdx.x; j < K; j += 256) co[j] = row[min(max(cand[(long)n * K + j], 0), V - 1)];
    __syncthreads();
    for (int i = threadIdx.x; i < V; i += 256) row[i] = (1.f - lam) * row[i] + lam * -1000000.0f;
    __syncthreads();
    for (int j = threadIdx.x; j < K; j += 256) {
        const float ctc_char = psi[(long)n * K + j] - prev_ctc[n];
        row[min(max(cand[(long)n * K + j], 0), V - 1)] = (1.f - lam) * co[j] + lam * ctc_char;
    }
    __syncthreads();
    if (threadIdx.x == 0) row[0] = -10000000.0f;
}

// Hypothesis.addTopk (postprocess.py:71-104) + the ranking of asr.py:237-252 for one utterance per workgroup.
struct SelectArgs {
    const float* topv; const int32_t* topi; const int32_t* cand;
    int U, beam, kb, K, step;
    const int32_t* n_live; const double* sum; const int32_t* plen; const int32_t* limit;
    int32_t *parent, *tok_new, *j_new, *plen_new; double* sum_new; int32_t *n_new, *rec;
};

constexpr int SELECT_NT = 512;                      // beam 20: one candidate per thread in the ranking pass

__global__ __launch_bounds__(SELECT_NT) void beam_select_kernel(SelectArgs a) {
    // LDS: per candidate its average score, token, score and a "may be expanded" flag; the live slots' candidate lists
    extern __shared__ double key[];                  // [beam*kb]
    const int NCmax = a.beam * a.kb;
    int32_t* valid = (int32_t*)(key + NCmax);        // [beam*kb] 1: expandable, 0: <eos>
    int32_t* ctok = valid + NCmax;                   // [beam*kb]
    float* csc = (float*)(ctok + NCmax);             // [beam*kb]
    int32_t* lcand = (int32_t*)(csc + NCmax);        // [beam][K]
    __shared__ int n_valid;
    const int u = blockIdx.x, beam = a.beam, kb = a.kb, K = a.K, row0 = u * beam;
    const long R = (long)a.U * beam;
    int32_t* rec_tok = a.rec;
    int32_t* rec_par = a.rec + R;
    float* rec_score = (float*)(a.rec + 2 * R);
    int32_t* rec_term = a.rec + 3 * R;
    float* rec_tscore = (float*)(a.rec + 4 * R);
    int32_t* rec_cnt = a.rec + 5 * R;
    const bool active = a.step < a.limit[u];
    const int nl = min(max(a.n_live[u], 0), beam);
    for (int s = threadIdx.x; s < beam; s += SELECT_NT) {
        rec_tok[row0 + s] = 0; rec_par[row0 + s] = 0; rec_score[row0 + s] = 0.f;
        rec_term[row0 + s] = 0; rec_tscore[row0 + s] = 0.f;
    }
    if (threadIdx.x == 0) n_valid = 0;
    __syncthreads();
    if (!active) {                                    // past this utterance's step limit: its survivors stay as they are
        if (threadIdx.x == 0) { a.n_new[u] = nl; rec_cnt[u] = -1; }
        return;
    }
    const int NC = nl * kb;                           // candidates in the reference's order: live slot, then i
    if (a.cand)
        for (int i = threadIdx.x; i < nl * K; i += SELECT_NT) lcand[i] = a.cand[(long)row0 * K + i];
    for (int c = threadIdx.x; c < NC; c += SELECT_NT) {
        const int row = row0 + c / kb;
        const int tk = a.topi[(long)row0 * kb + c];
        const float sc = a.topv[(long)row0 * kb + c];
        ctok[c] = tk; csc[c] = sc;
        if (tk == 1) {                                // <eos>: the hypothesis terminates with this score, no expansion
            valid[c] = 0;
            key[c] = 0.0;
            rec_term[row] = 1;
            rec_tscore[row] = sc;
        } else {
            valid[c] = 1;
            key[c] = (a.sum[row] + (double)sc) / (double)(a.plen[row] + 1);
            atomicAdd(&n_valid, 1);
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < NC; c += SELECT_NT) {
        if (!valid[c]) continue;
        const double k = key[c];
        int rank = 0;                                 // candidates that sort before c (descending, stable)
        for (int o = 0; o < NC; ++o) {
            const double ko = key[o];
            rank += valid[o] & ((ko > k) | ((ko == k) & (o < c)));
        }
        if (rank >= beam) continue;
        const int s = c / kb, row = row0 + s, tk = ctok[c];
        const float sc = csc[c];
        int j = 0;
        if (a.cand)                                   // cand.index(tk)
            for (int q = K - 1; q >= 0; --q) j = lcand[s * K + q] == tk ? q : j;
        const int o = row0 + rank;
        a.parent[o] = s; a.tok_new[o] = tk; a.j_new[o] = j;
        a.plen_new[o] = a.plen[row] + 1;
        a.sum_new[o] = a.sum[row] + (double)sc;
        rec_tok[o] = tk; rec_par[o] = s; rec_score[o] = sc;
    }
    if (threadIdx.x == 0) {
        const int nn = min(n_valid, beam);
        a.n_new[u] = nn;
        rec_cnt[u] = nn;
    }
}

struct GatherArgs {
    int U, beam, NL, C, Tmax, K, step;
    const int32_t *T_u, *limit, *n_new, *parent, *j_new, *tok_new, *plen_new; const double* sum_new;
    float *hs, *cs, *att; const float *r_out, *psi; float *r_prev, *prev_ctc;
    int32_t *tok, *plen; double* sum; int32_t* n_live;
};

// one workgroup per new slot: state of the parent (slot 1 / the step's outputs) -> state the next step reads (slot 0)
__global__ __launch_bounds__(256) void beam_gather_kernel(GatherArgs a) {
    const int r = blockIdx.x, u = r / a.beam, s = r % a.beam;
    if (a.step >= a.limit[u]) return;
    const int nn = min(max(a.n_new[u], 0), a.beam);
    if (s == 0 && threadIdx.x == 0) a.n_live[u] = nn;
    if (s >= nn) return;
    const long R = (long)a.U * a.beam;
    const int ps = min(max(a.parent[r], 0), a.beam - 1);
    const long p = (long)u * a.beam + ps;
    const int C = a.C, Tm = a.Tmax;
    for (int l = 0; l < a.NL; ++l) {
        const float* hsrc = a.hs + ((long)(2 * l + 1) * R + p) * C;
        const float* csrc = a.cs + ((long)(2 * l + 1) * R + p) * C;
        float* hdst = a.hs + ((long)(2 * l) * R + r) * C;
        float* cdst = a.cs + ((long)(2 * l) * R + r) * C;
        for (int i = threadIdx.x; i < C; i += 256) { hdst[i] = hsrc[i]; cdst[i] = csrc[i]; }
    }
    if (a.att)
        for (int i = threadIdx.x; i < Tm; i += 256) a.att[(long)r * Tm + i] = a.att[(R + p) * Tm + i];
    if (a.r_out) {
        const int j = min(max(a.j_new[r], 0), a.K - 1);
        const int T = min(max(a.T_u[u], 1), Tm);
        const float* src = a.r_out + (p * a.K + j) * Tm * 2;
        float* dst = a.r_prev + (long)r * Tm * 2;
        for (int i = threadIdx.x; i < 2 * T; i += 256) dst[i] = src[i];
        if (threadIdx.x == 0) a.prev_ctc[r] = a.psi[p * a.K + j];
    }
    if (threadIdx.x == 0) { a.tok[r] = a.tok_new[r]; a.plen[r] = a.plen_new[r]; a.sum[r] = a.sum_new[r]; }
}

}  // namespace

extern "C" int las_log_softmax_rows(const float* x, int R, int V, float* out, void* stream) {
    LAS_CHECK_ARG(x && out && R >= 0 && V > 0);
    if (R == 0) return LAS_OK;
    hipLaunchKernelGGL(log_softmax_rows_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, x, V, out);
    LAS_LAUNCH_OK();
    return LAS_OK;
}

extern "C" int las_topk_rows(const float* x, int R, int V, int k, float* vals, int32_t* idx, void* stream) {
    LAS_CHECK_ARG(x && vals && idx && R >= 0 && V > 0 && k > 0 && k <= V);
    if ((size_t)V * sizeof(float) > 60 * 1024) return LAS_E_UNSUPPORTED;
    if (R == 0) return LAS_OK;
    hipLaunchKernelGGL(topk_rows_kernel, dim3(R), dim3(256), sizeof(float) * V, (hipStream_t)stream, x, V, k, vals, idx);
    LAS_LAUNCH_OK();
    return LAS_OK;
}

extern "C" int las_ctc_prefix_init(const float* lp, int T, int V, float* r0, void* stream) {
    LAS_CHECK_ARG(lp && r0 && T > 0 && V > 1);
    hipLaunchKernelGGL(ctc_prefix_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, lp, T, V, r0);
    LAS_LAUNCH_OK();
    return LAS_OK;
}

extern "C" int las_ctc_prefix_score(const float* lp, int T, int V, const float* r_prev, const int32_t* last_tok,
                                    const int32_t* prefix_len, const int32_t* cand, int N, int K, float* psi, float* r_out,
                                    void* stream) {
    LAS_CHECK_ARG(lp && r_prev && last_tok && prefix_len && cand && psi && r_out && T > 0 && V > 1 && N >= 0 && K > 0);
    if (N == 0) return LAS_OK;
    hipLaunchKernelGGL(ctc_prefix_score_kernel, dim3((N * K + 63) / 64), dim3(64), 0, (hipStream_t)stream, lp, T, V, r_prev,
                       last_tok, prefix_len, cand, N, K, psi, r_out);
    LAS_LAUNCH_OK();
    return LAS_OK;
}

extern "C" int las_beam_combine(float* cur, int N, int V, const int32_t* cand, const float* psi, const float* prev_ctc, int K,
                                float ctc_weight, void* stream) {
    LAS_CHECK_ARG(cur && cand && psi && prev_ctc && N >= 0 && V > 1 && K > 0 && K <= V);
    if (N == 0) return LAS_OK;
    hipLaunchKernelGGL(beam_combine_kernel, dim3(N), dim3(256), sizeof(float) * K, (hipStream_t)stream, cur, V, cand, psi,
                       prev_ctc, K, ctc_weight);
    LAS_LAUNCH_OK();
    return LAS_OK;
}

extern "C" int las_ctc_prefix_init_batch(const float* lp, int U, int Tmax, int V, const int32_t* T_u, float* r0, void* stream) {
    LAS_CHECK_ARG(lp && T_u && r0 && U >= 0 && Tmax > 0 && V > 1);
    if (U == 0) return LAS_OK;
    hipLaunchKernelGGL(ctc_prefix_init_batch_kernel, dim3((U + 63) / 64), dim3(64), 0, (hipStream_t)stream, lp, U, Tmax, V, T_u, r0);
    LAS_LAUNCH_OK();
    return LAS_OK;
}

extern "C" int las_ctc_prefix_score_batch(const float* lp, int U, int Tmax, int V, const int32_t* T_u, const int32_t* row_utt,
                                          const float* r_prev, const int32_t* last_tok, const int32_t* prefix_len,
                                          const int32_t* cand, int N, int K, float* psi, float* r_out, void* stream) {
    LAS_CHECK_ARG(lp && T_u && row_utt && r_prev && last_tok && prefix_len && cand && psi && r_out && U > 0 && Tmax > 0 &&
                  V > 1 && N >= 0 && K > 0);
    if (N == 0) return LAS_OK;
    hipLaunchKernelGGL(ctc_prefix_score_batch_kernel, dim3((N * K + 63) / 64), dim3(64), 0, (hipStream_t)stream, lp, Tmax, V, U,
                       T_u, row_utt, r_prev, last_tok, prefix_len, cand, N, K, psi, r_out);
    LAS_LAUNCH_OK();
    return LAS_OK;
}

extern "C" int las_beam_select(const float* topv, const int32_t* topi, const int32_t* cand, int U, int beam, int kb, int K,
                               const int32_t* n_live, const double* sum, const int32_t* plen, const int32_t* limit, int step,
                               int32_t* parent, int32_t* tok_new, int32_t* j_new, int32_t* plen_new, double* sum_new,
                               int32_t* n_new, int32_t* rec, void* stream) {
    LAS_CHECK_ARG(topv && topi && n_live && sum && plen && limit && parent && tok_new && j_new && plen_new && sum_new && n_new &&
                  rec && U >= 0 && beam > 0 && kb > 0 && kb <= beam && step >= 0 && (!cand || K > 0));
    if (U == 0) return LAS_OK;
    const size_t lds = (size_t)beam * kb * (sizeof(double) + 3 * sizeof(int32_t)) + (cand ? (size_t)beam * K * sizeof(int32_t) : 0);
    if (lds > 60 * 1024) return LAS_E_UNSUPPORTED;
    SelectArgs a{topv, topi, cand, U, beam, kb, K, step, n_live, sum, plen, limit, parent, tok_new, j_new, plen_new, sum_new, n_new, rec};
    hipLaunchKernelGGL(beam_select_kernel, dim3(U), dim3(SELECT_NT), lds, (hipStream_t)stream, a);
    LAS_LAUNCH_OK();
    return LAS_OK;
}

extern "C" int las_beam_gather(int U, int beam, int NL, int C, int Tmax, int K, const int32_t* T_u, const int32_t* limit, int step,
                               const int32_t* n_new, const int32_t* parent, const int32_t* j_new, const int32_t* tok_new,
                               const int32_t* plen_new, const double* sum_new, float* hs, float* cs, float* att,
                               const float* r_out, const float* psi, float* r_prev, float* prev_ctc, int32_t* tok, int32_t* plen,
                               double* sum, int32_t* n_live, void* stream) {
    LAS_CHECK_ARG(limit && n_new && parent && j_new && tok_new && plen_new && sum_new && hs && cs && tok && plen && sum && n_live &&
                  U >= 0 && beam > 0 && NL >= 1 && C > 0 && Tmax > 0 && step >= 0);
    LAS_CHECK_ARG(!r_out || (psi && r_prev && prev_ctc && T_u && K > 0));
    if (U == 0) return LAS_OK;
    GatherArgs a{U, beam, NL, C, Tmax, K, step, T_u, limit, n_new, parent, j_new, tok_new, plen_new, sum_new,
                 hs, cs, att, r_out, psi, r_prev, prev_ctc, tok, plen, sum, n_live};
    hipLaunchKernelGGL(beam_gather_kernel, dim3(U * beam), dim3(256), 0, (hipStream_t)stream, a);
    LAS_LAUNCH_OK();
    return LAS_OK;
}
