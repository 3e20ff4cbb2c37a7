// fp32-mode persistent (Bi)LSTM recurrence / BPTT for hidden sizes whose f32 W_hh slab does not fit the CU's LDS
// (H > ~490 at one batch tile per slice, H > ~400 at two; up to H = 1024) -- included by lstm.hip inside its anonymous
// namespace (reference: the sequential half of nn.LSTM at src/asr.py:473-481 and its autograd, fp32 throughout).
//
// Same ownership, data flow, saved layouts (gates / cs / hf / dgf) and hand-off as the f32 instances of lstm_fwd_kernel and
// lstm_bwd_ks_kernel: block_signal / block_wait, sc1 stores, drain, one counter per (direction, slice), the HX_SLOTS /
// KS_SLOTS rings.  What differs is where the weights live: in REGISTERS, as f32 MFMA fragments fetched from global memory
// once per launch.
//   forward : wave w <-> gate w; lane (fr, fq) keeps W_hh[gate w][unit j0 + fr][k = 16 ks + 4 fq + {0..3}] for every k-step:
//             4 KS floats per lane (KS = 64 at H = 1024: 256 of the 512 registers a lane owns with one wave per SIMD).
//   backward: K-split; wave w takes consumers c = w, w + 4, ...; lane (fr, fq) keeps W_hh[k][column 16 c + fr] of the
//             workgroup's own 64 gate rows (k = gate * 16 + unit = 16 ks + 4 fq + {0..3}): 16 MT floats per lane (MT = 16 at
//             H = 1024: again 256).
// The h tile / the inbox of partial d h take the LDS the slab had ([16 NB][H + 4] f32 = 66 KB per batch tile at H = 1024), so
// a split placement (part of every row in LDS) has nothing left at two batch tiles per slice; at one tile (22 of the 64
// k-steps in a 91 KB slab, 168 weight registers) it measured 3-4 % faster forward and was not kept: the
// register form serves one and two tiles alike.  Products and sums are exact fp32 (v_mfma_f32_16x16x4_f32); every dot product runs as two
// interleaved accumulator chains (the instruction's dependent latency is 40 cycles against an issue interval of 32).
// One and two batch tiles per slice, even H <= 1024.

template <int NB, int KS>       // KS: k-steps of 16 held per lane (>= ceil(H / 16); steps beyond it hold zero weights)
__global__ __launch_bounds__(NT) void lstm_fwd_f32w_kernel(LstmArgs a, const float* __restrict__ xproj,
                                                           const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                                                           const float* __restrict__ w_hh, const int32_t* __restrict__ lens,
                                                           float* __restrict__ y, float* __restrict__ hf,
                                                           float* __restrict__ hx, float* __restrict__ gates,
                                                           float* __restrict__ cs, SyncWords* sync, int* status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int H = a.H, B = a.B, ND = a.ND;
    const int Kp = (H + 15) / 16 * 16, ld = Kp + 4;
    const int Hx = (H + 3) / 4 * 4;                     // exchange row stride (pad columns are caller-zeroed)
    const Role role = lstm_role(a);
    if (role.idle) return;
    const int d = role.d, g = role.g, bs = role.bs, j0 = g * 16;
    const int b0 = bs * a.Bs, Bl = min(a.Bs, B - b0);
    float* Hl = (float*)smem;                           // [NB*16][ld]; pad rows / columns stay zero
    float* Gl = Hl + NB * 16 * ld;                      // [4][NB*16][17]
    int* lensl = (int*)(Gl + 4 * NB * 16 * 17);         // [NB*16]
    int* flag = lensl + NB * 16;
    for (int i = threadIdx.x; i < NB * 16 * ld; i += NT) Hl[i] = 0.f;
    for (int i = threadIdx.x; i < NB * 16; i += NT) lensl[i] = i < Bl ? lens[b0 + i] : 0;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, fr = lane & 15, fq = lane >> 4;
    // the wave's weight fragments, for all T steps
    float wr[KS][4];
    {
        const bool rowok = j0 + fr < H;
        const float* wrow = w_hh + ((long)d * 4 * H + wave * H + min(j0 + fr, H - 1)) * H;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int c = ks * 16 + fq * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = wrow[min(c + e, H - 1)];
                wr[ks][e] = (rowok && c + e < H) ? v : 0.f;
            }
        }
    }
    // pointwise elements: ONE (batch row, unit) per thread and 256-element pass, as in lstm_fwd_kernel
    constexpr int PE = NB;
    float c_state[PE];
    float bias[PE][4];
    int eb[PE], en[PE];
    bool ev[PE];
#pragma unroll
    for (int p = 0; p < PE; ++p) {
        const int e = threadIdx.x + p * NT;
        eb[p] = e >> 4; en[p] = e & 15;
        ev[p] = eb[p] < Bl && (j0 + en[p] < H);
        c_state[p] = 0.f;
#pragma unroll
        for (int gi = 0; gi < 4; ++gi) {
            const int j = j0 + en[p];
            bias[p][gi] = ev[p] ? b_ih[d * 4 * H + gi * H + j] + b_hh[d * 4 * H + gi * H + j] : 0.f;
        }
    }
    const int ND4H = ND * 4 * H;
    unsigned* cnt = &sync->cnt[(d * MAX_SLICES + bs) * CNT_STRIDE];
    const int gl = group_local(a, cnt, &sync->abort_, flag);
    if (gl < 0) { if (threadIdx.x == 0) *status = LAS_E_TIMEOUT; return; }
    const bool local = gl == 1;

    for (int s = 0; s < a.T; ++s) {
        const int t = d == 0 ? s : a.T - 1 - s;
        float xp[PE][4];
#pragma unroll
        for (int p = 0; p < PE; ++p)
#pragma unroll
            for (int gi = 0; gi < 4; ++gi)
                xp[p][gi] = ev[p] ? xproj[((long)t * B + b0 + eb[p]) * ND4H + d * 4 * H + gi * H + j0 + en[p]] : 0.f;
        f32x4 acc[NB][2];
#pragma unroll
        for (int bt = 0; bt < NB; ++bt) acc[bt][0] = acc[bt][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (s > 0) {
            if (!block_wait(cnt, a.G, (unsigned)s, &sync->abort_, flag, local)) { if (threadIdx.x == 0) *status = LAS_E_TIMEOUT; return; }
            pull_tile_sc1<float, 4, 8>(hx + (((long)d * HX_SLOTS + ((s - 1) & (HX_SLOTS - 1))) * B + b0) * Hx, Bl, Hx, Hx, 0, Hl, ld);
            __syncthreads();
            // gate pre-activations: h fragments from LDS in chunks of CH k-steps (a k-step beyond Kp re-reads the last one
            // against zero weights), weights from registers
            constexpr int CH = 8;
#pragma unroll
            for (int k0 = 0; k0 < KS; k0 += CH) {
                float4 av[CH][NB];
#pragma unroll
                for (int ks = 0; ks < CH; ++ks)
#pragma unroll
                    for (int bt = 0; bt < NB; ++bt)
                        av[ks][bt] = *(const float4*)(Hl + (bt * 16 + fr) * ld + min((k0 + ks) * 16, Kp - 16) + fq * 4);
#pragma unroll
                for (int ks = 0; ks < CH; ++ks)
#pragma unroll
                    for (int bt = 0; bt < NB; ++bt) {
                        acc[bt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ks][bt].x, wr[k0 + ks][0], acc[bt][0], 0, 0, 0);
                        acc[bt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ks][bt].y, wr[k0 + ks][1], acc[bt][1], 0, 0, 0);
                        acc[bt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ks][bt].z, wr[k0 + ks][2], acc[bt][0], 0, 0, 0);
                        acc[bt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ks][bt].w, wr[k0 + ks][3], acc[bt][1], 0, 0, 0);
                    }
            }
        }
        // accumulators -> LDS  (C/D layout: col = lane&15 = unit, row = (lane>>4)*4 + r = batch)
#pragma unroll
        for (int bt = 0; bt < NB; ++bt)
#pragma unroll
            for (int r = 0; r < 4; ++r) Gl[(wave * NB * 16 + bt * 16 + fq * 4 + r) * 17 + fr] = acc[bt][0][r] + acc[bt][1][r];
        __syncthreads();
        // pointwise cell update; publish h_t FIRST, signal, then write what only the backward pass reads
        float hv[PE], gv[PE][4];
#pragma unroll
        for (int p = 0; p < PE; ++p) {
            const int bl = min(eb[p], NB * 16 - 1), n = en[p], j = j0 + n;
            const bool mq = ev[p] && t < lensl[bl];
            const float pi = Gl[(0 * NB * 16 + bl) * 17 + n] + xp[p][0] + bias[p][0];
            const float pf = Gl[(1 * NB * 16 + bl) * 17 + n] + xp[p][1] + bias[p][1];
            const float pg = Gl[(2 * NB * 16 + bl) * 17 + n] + xp[p][2] + bias[p][2];
            const float po = Gl[(3 * NB * 16 + bl) * 17 + n] + xp[p][3] + bias[p][3];
            const float ig = fsig(pi), fg = fsig(pf), gg = ftanh(pg), og = fsig(po);
            const float cn = fg * c_state[p] + ig * gg;
            const float hn = og * ftanh(cn);
            c_state[p] = mq ? cn : c_state[p];
            hv[p] = mq ? hn : 0.f;
            gv[p][0] = mq ? ig : 0.f; gv[p][1] = mq ? fg : 0.f; gv[p][2] = mq ? gg : 0.f; gv[p][3] = mq ? og : 0.f;
            // the unit pair (n, n+1) goes out as one store from the even lane; its partner's h comes over DPP (row_shl:1)
            const float hnext = las_dpp<0x101, 0xf>(0.f, hv[p]);
            if (ev[p] && !(n & 1)) st_pair_x(hx + (((long)d * HX_SLOTS + (s & (HX_SLOTS - 1))) * B + b0 + bl) * Hx + j, hv[p], hnext, local);
        }
        block_signal(cnt, local, g, (unsigned)s + 1u);
#pragma unroll
        for (int p = 0; p < PE; ++p) {
            if (!ev[p]) continue;
            const int bl = eb[p], b = b0 + bl, j = j0 + en[p];
            const bool m = t < lensl[bl];
            const long ro = (long)t * B + b;
            // (write-only streams read by later kernels: non-temporal, so they neither wait for nor keep L2 lines)
            __builtin_nontemporal_store(hv[p], &hf[ro * (ND * H) + d * H + j]);
            if (!a.y_is_hf) {
                bool ok;
                const long yo = y_offset(a, t, b, d, j, ok);
                if (ok) __builtin_nontemporal_store(hv[p], &y[yo]);
            }
#pragma unroll
            for (int gi = 0; gi < 4; ++gi) __builtin_nontemporal_store(gv[p][gi], &gates[ro * ND4H + d * 4 * H + gi * H + j]);
            __builtin_nontemporal_store(m ? c_state[p] : 0.f, &cs[ro * (ND * H) + d * H + j]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward, K-split
template <int NB, int MT>     // MT = consumers (16-column tiles) per wave >= ceil(G / 4)
__global__ __launch_bounds__(NT) void lstm_bwd_f32w_kernel(LstmArgs a, const float* __restrict__ dy,
                                                           const float* __restrict__ gates, const float* __restrict__ cs,
                                                           const float* __restrict__ w_hh, const int32_t* __restrict__ lens,
                                                           unsigned* __restrict__ pex, float* __restrict__ dgf,
                                                           SyncWords* sync, int* status) {
    constexpr int KO = 64, LDK = KO + 4;                  // own dgates: k = gate*16 + unit
    constexpr int WPR = 16;                               // exchange words per batch row of a 16-column piece
    constexpr int WPT = NB * 16 * WPR;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int H = a.H, B = a.B, ND = a.ND, K4 = 4 * H, G = a.G;
    const Role role = lstm_role(a);
    if (role.idle) return;
    const int d = role.d, g = role.g, bs = role.bs, j0 = g * 16;
    const int b0 = bs * a.Bs, Bl = min(a.Bs, B - b0);
    float* Dl = (float*)smem;                             // [NB*16][LDK] my dgates of this step
    unsigned* Pl = (unsigned*)(Dl + NB * 16 * LDK);       // [G][WPT] inbox of the previous step
    int* lensl = (int*)(Pl + (size_t)G * WPT);
    int* flag = lensl + NB * 16;
    for (int i = threadIdx.x; i < NB * 16 * LDK; i += NT) Dl[i] = 0.f;
    for (int i = threadIdx.x; i < NB * 16; i += NT) lensl[i] = i < Bl ? lens[b0 + i] : 0;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, fr = lane & 15, fq = lane >> 4;
    // The product is taken transposed (A = W rows = output columns, B = dgates rows = batch), so a lane ends up with
    // FOUR CONSECUTIVE output columns of one batch row: one 16-byte store per tile.
    // element 4 ks + e <-> k = 16 ks + 4 fq + e = gate ks, unit 4 fq + e; output column 16 c + fr
    float wr[MT][16];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int col = min(wave + 4 * i, G - 1) * 16 + fr;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int n = 4 * fq + e;
                const float v = w_hh[((long)d * K4 + ks * H + min(j0 + n, H - 1)) * H + min(col, H - 1)];
                wr[i][ks * 4 + e] = (col < H && j0 + n < H) ? v : 0.f;
            }
    }

    // pointwise elements of this thread: the pair (row eb, units en, en+1)  (NB <= 2: at most one pair per thread)
    const int e = threadIdx.x, eb = e >> 3, en = (e & 7) * 2, j = j0 + en;
    const bool ev = e < NB * 16 * 8 && eb < Bl && j < H;
    float dc_carry[2] = {0.f, 0.f};
    const int ND4H = ND * K4, NDH = ND * H;
    unsigned* cnt = &sync->cnt[(d * MAX_SLICES + bs) * CNT_STRIDE];
    const long slot_words = (long)ND * a.NS * G * G * WPT;
    auto inbox = [&](int slot, int consumer, int producer) -> unsigned* {
        return pex + slot * slot_words + ((((long)d * a.NS + bs) * G + consumer) * G + producer) * WPT;
    };
    // saved activations / incoming gradient of one step, requested a step ahead of their use
    float2 sg[4], sc, scp, sdy;
    auto load_inputs = [&](int s) {
        const int t = d == 0 ? a.T - 1 - s : s, tp = d == 0 ? t - 1 : t + 1;
        sc = scp = sdy = make_float2(0.f, 0.f);
#pragma unroll
        for (int gi = 0; gi < 4; ++gi) sg[gi] = make_float2(0.f, 0.f);
        if (!ev || s >= a.T || t >= lensl[eb]) return;
        const int b = b0 + eb;
        const long ro = (long)t * B + b;
#pragma unroll
        for (int gi = 0; gi < 4; ++gi) sg[gi] = *(const float2*)(gates + ro * ND4H + d * K4 + gi * H + j);
        sc = *(const float2*)(cs + ro * NDH + d * H + j);
        if (tp >= 0 && tp < lensl[eb]) scp = *(const float2*)(cs + ((long)tp * B + b) * NDH + d * H + j);
        bool ok;
        const long yo = y_offset(a, t, b, d, j, ok);
        if (ok) sdy = *(const float2*)(dy + yo);
    };
    load_inputs(0);
    const int gl = group_local(a, cnt, &sync->abort_, flag);
    if (gl < 0) { if (threadIdx.x == 0) *status = LAS_E_TIMEOUT; return; }
    const bool local = gl == 1;

    for (int s = 0; s < a.T; ++s) {
        const int t = d == 0 ? a.T - 1 - s : s;           // reverse of the forward processing order
        float dh_rec[2] = {0.f, 0.f};
        if (s > 0) {
            if (!block_wait(cnt, G, (unsigned)s, &sync->abort_, flag, local)) { if (threadIdx.x == 0) *status = LAS_E_TIMEOUT; return; }
            // (only the Bl batch rows of each piece that carry data are pulled)
            pull_tile_sc1<unsigned, 4, 8>(inbox((s - 1) & (KS_SLOTS - 1), g, 0), G, Bl * WPR, WPT, 0, Pl, WPT);
            __syncthreads();
            if (ev) {                                     // sum of the G pieces, four chains
                const unsigned* pw = Pl + eb * WPR + en;
                float s0[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f};
                int p = 0;
                for (; p + 3 < G; p += 4) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const uint2 w = *(const uint2*)(pw + (p + u) * WPT);
                        s0[u] += __uint_as_float(w.x);
                        s1[u] += __uint_as_float(w.y);
                    }
                }
                for (; p < G; ++p) {
                    const uint2 w = *(const uint2*)(pw + p * WPT);
                    s0[0] += __uint_as_float(w.x);
                    s1[0] += __uint_as_float(w.y);
                }
                dh_rec[0] = (s0[0] + s0[1]) + (s0[2] + s0[3]);
                dh_rec[1] = (s1[0] + s1[1]) + (s1[2] + s1[3]);
            }
        }
        // pointwise BPTT -> my dgates of this step, into LDS for the product below
        float dg[4][2];
        {
            const bool m = ev && t < lensl[min(eb, NB * 16 - 1)];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const float ig = q ? sg[0].y : sg[0].x, fg = q ? sg[1].y : sg[1].x;
                const float gg = q ? sg[2].y : sg[2].x, og = q ? sg[3].y : sg[3].x;
                const float ct = q ? sc.y : sc.x, cp = q ? scp.y : scp.x;
                const float dh = (q ? sdy.y : sdy.x) + dh_rec[q];
                const float tc = ftanh(ct);
                const float dc = dh * og * (1.f - tc * tc) + dc_carry[q];
                const bool mq = m && (j + q < H);
                dg[0][q] = mq ? dc * gg * ig * (1.f - ig) : 0.f;
                dg[1][q] = mq ? dc * cp * fg * (1.f - fg) : 0.f;
                dg[2][q] = mq ? dc * ig * (1.f - gg * gg) : 0.f;
                dg[3][q] = mq ? dh * tc * og * (1.f - og) : 0.f;
                dc_carry[q] = mq ? dc * fg : 0.f;
            }
            if (ev) {
#pragma unroll
                for (int gi = 0; gi < 4; ++gi) *(float2*)(Dl + eb * LDK + gi * 16 + en) = make_float2(dg[gi][0], dg[gi][1]);
            }
        }
        __syncthreads();
        if (s + 1 < a.T) {
            // partial dh_{t-1}[:, 16 c .. 16 c + 15] for every consumer c; wave w takes c = w, w+4, ...
            const int slot = s & (KS_SLOTS - 1);
            float4 dv[NB][4];
#pragma unroll
            for (int bt = 0; bt < NB; ++bt)
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) dv[bt][ks] = *(const float4*)(Dl + (bt * 16 + fr) * LDK + ks * 16 + fq * 4);
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int c = wave + 4 * i;
                if (c >= G) break;
                unsigned* dst = inbox(slot, c, g);
                __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)dst, 0, WPT * 4, 0x00020000);
#pragma unroll
                for (int bt = 0; bt < NB; ++bt) {
                    f32x4 a0 = (f32x4){0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) {
                        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[i][ks * 4 + 0], dv[bt][ks].x, a0, 0, 0, 0);
                        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[i][ks * 4 + 1], dv[bt][ks].y, a1, 0, 0, 0);
                        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[i][ks * 4 + 2], dv[bt][ks].z, a0, 0, 0, 0);
                        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[i][ks * 4 + 3], dv[bt][ks].w, a1, 0, 0, 0);
                    }
                    // lane: batch row bt*16 + fr, output columns 16c + 4 fq + {0..3}
                    const int row = bt * 16 + fr;
                    if (row < Bl) {
                        const u32x4 v = {__float_as_uint(a0[0] + a1[0]), __float_as_uint(a0[1] + a1[1]), __float_as_uint(a0[2] + a1[2]),
                                         __float_as_uint(a0[3] + a1[3])};
                        if (local) __builtin_amdgcn_raw_buffer_store_b128(v, rs, (row * WPR + fq * 4) * 4, 0, 0);
                        else __builtin_amdgcn_raw_buffer_store_b128(v, rs, (row * WPR + fq * 4) * 4, 0, 16);
                    }
                }
            }
            block_signal(cnt, local, g, (unsigned)s + 1u);
        }
        // fp32 copy for the weight-gradient GEMMs, then next step's inputs
        if (ev) {
            const long ro = (long)t * B + b0 + eb;
#pragma unroll
            for (int gi = 0; gi < 4; ++gi)
                *(float2*)(dgf + ro * ND4H + d * K4 + gi * H + j) = make_float2(dg[gi][0], dg[gi][1]);
        }
        load_inputs(s + 1);
    }
}

// LDS requests (bytes) and the shapes these kernels take: fp32 mode, one or two batch tiles per slice, H <= 1024.
size_t fwd_f32w_lds(int H, int NB) {
    const int Kp = (H + 15) / 16 * 16, ld = Kp + 4;
    return sizeof(float) * ((size_t)NB * 16 * ld + 4 * NB * 16 * 17) + sizeof(int) * (NB * 16 + 4);
}
size_t bwd_f32w_lds(int H, int NB) {
    const int G = (H + 15) / 16;
    return sizeof(float) * (size_t)NB * 16 * (64 + 4) + sizeof(unsigned) * (size_t)G * ks_words_per_tile(LAS_PREC_F32, NB) +
           sizeof(int) * (NB * 16 + 4);
}
bool f32w_ok(int prec, int H, int NB) { return prec == LAS_PREC_F32 && H <= 1024 && NB >= 1 && NB <= 2; }
