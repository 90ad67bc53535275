// The one-wave LSTM recurrence bodies (H <= 16), shared by lstm.hip (stand-alone kernels) and gemm.hip (riders of a
// gemm_kernel launch), with the gate activations and vector types they and the other LSTM kernels use.
#pragma once
#include "mst_common.h"

__device__ __forceinline__ float sigm(float x) { return MST_FAST_RCP(1.f + MST_FAST_EXP(-x)); }
__device__ __forceinline__ float tanh_fast(float x) { return 2.f * sigm(2.f * x) - 1.f; }

typedef float lstm_f4 __attribute__((ext_vector_type(4)));
typedef float lstm_f4u __attribute__((ext_vector_type(4), aligned(4)));       // a 16-byte load from a 4-byte aligned address


// ---- one-wave flavour (H <= LSTM_SH) --------------------------------------------------------------
// The song-info model's two LSTMs (H = 9 over the beats of a bar, H = 8 over the bars) have G = 4H <= 64 gate rows: the register
// flavour above, laid out for H = 64, spends 64 FMAs per lane, two s_barriers and two LDS exchanges (h_s -> z_s -> gate lanes) on
// a step that holds a few hundred multiply-adds.  Here ONE wave runs a sequence: lane u < H owns hidden unit u and does the
// unit's whole step — all four gate pre-activations out of its own rows q H + u of W_hh (forward), dh_{t-1}[u] out of its own
// column of all four parts (backward) — so the only exchange of a step is the broadcast of h_{t-1} / dz_t through a
// wave-private LDS slice (MST_WAVE_SYNC: no s_barrier anywhere).  The streamed operands of as many steps as the slice holds are
// staged at once, the first chunk together with the weight and bias loads.  The bodies take the wave's LDS slice and lane as
// arguments: they do not care which kernel the wave belongs to.
// Per sequence the arithmetic, its order and its roundings are those of lstm_fwd_kernel<true> / lstm_bwd_kernel<true> as the
// gfx950 build has always evaluated them: bit-identical results.  That includes what hipcc contracts there (1 - x * x and the
// cell gradient's multiply-add: one fma each) and what it does not (the cell update fg * c + ig * gg: it packs the two products
// into one v_pk_mul_f32 and adds), written out below so that neither depends on what the compiler vectorises around them.
#define LSTM_SH 16            // largest H of the one-wave flavour
#define LSTM_SW_X 64          // floats of a wave's slice for the per-step exchange: h_{t-1}, or dz_t with a part every 16 floats
#define LSTM_SW_LDS 1024      // floats of a wave's slice; behind the exchange: the staged operands
// a * b + c as ONE fma on the device and as two roundings in the interpreter, whose x86-64 build does not contract (see
// lstm_multi_bwd_kernel)
#ifdef HIPSIM
#define LSTM_MULADD(a, b, c) ((a) * (b) + (c))
#else
#define LSTM_MULADD(a, b, c) __builtin_fmaf((a), (b), (c))
#endif
__device__ __forceinline__ float lstm_cell_update(const float fg, const float c, const float ig, const float gg) {
#pragma clang fp contract(off)
    const float keep = fg * c, add = ig * gg;       // two roundings, then the sum's
    return keep + add;
}

// WL (the rider form: a wave of gemm_kernel has no registers for 4 KP weights): W_hh waits in the wave's slice, zero-padded to
// KP x KP per gate — forward w_s[(q KP + k) KP + u] = W_hh[q H + u, k], backward w_s[(p KP + jj) KP + u] = W_hh[p H + jj, u] — so a
// step reads its weights with lanes along u (conflict-free) at compile-time offsets.  Filled coalesced: lane l takes the flat
// elements l, l + 64, ... (all loads in flight, one wait); (row, column) advance without a division per element.
#define LSTM_WL_F(KP) (4 * (KP) * (KP))
template <int KP, bool BWD>
__device__ __forceinline__ void lstm_small_stage_whh(const MST_GLOBAL_AS float* whh, const int H, const int u, float* w_s) {
    constexpr int N = LSTM_WL_F(KP) / 64;          // KP = 8: 4, KP = 12: 9 — at least 4 H H / 64 elements per lane
#pragma unroll
    for (int i = 0; i < N; ++i) w_s[u + 64 * i] = 0.f;
    MST_WAVE_SYNC();
    const int total = 4 * H * H, dq = 64 / H, dr = 64 - dq * H;
    float t[N];
#pragma unroll
    for (int i = 0; i < N; ++i) t[i] = whh[min(u + 64 * i, total - 1)];
    int row = u / H, col = u - row * H;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int g = (row >= H) + (row >= 2 * H) + (row >= 3 * H), rr = row - g * H;
        if (u + 64 * i < total) w_s[BWD ? (g * KP + rr) * KP + col : (g * KP + col) * KP + rr] = t[i];
        row += dq; col += dr;
        if (col >= H) { col -= H; ++row; }
    }
}

// KP: the launch's largest H rounded up to a multiple of 4 (the k range of the four FMA chains; weights beyond H are zero)
template <int KP, bool WL = false>
__device__ __forceinline__ void lstm_small_fwd_body(const LstmDesc& d, const int bi, const int u, const Bases& b, float* lds) {
    const int H = d.H, G = 4 * d.H;
    float* x_s = lds;                              // h_{t-1}[k], zero for k >= H
    float* w_s = lds + LSTM_SW_X;                  // WL: the weights
    float* zx_s = lds + LSTM_SW_X + (WL ? LSTM_WL_F(KP) : 0);      // zx rows of the next zchunk steps
    const int zchunk = (LSTM_SW_LDS - LSTM_SW_X - (WL ? LSTM_WL_F(KP) : 0)) / G;
    const MST_GLOBAL_AS float* whh = (const MST_GLOBAL_AS float*)(b.p[SP_PAR] + d.whh_off);
    const MST_GLOBAL_AS float* bhh = (const MST_GLOBAL_AS float*)(b.p[SP_PAR] + d.bhh_off);
    const MST_GLOBAL_AS float* zx = (const MST_GLOBAL_AS float*)(b.p[SP_WS] + d.zx_off) + (int64_t)bi * d.S * G;
    MST_GLOBAL_AS float* ws = (MST_GLOBAL_AS float*)b.p[SP_WS];
    MST_GLOBAL_AS float* tmp = (MST_GLOBAL_AS float*)b.p[SP_TMP];
    // rows q H + u of W_hh as 16-byte loads from 4-byte aligned addresses, clamped to end inside the matrix (lstm_fwd_kernel)
    lstm_f4u wv[WL ? 1 : 4][WL ? 1 : KP / 4];
    const int wlast = max(G * H - 4, 0);
    const int uc = min(u, H - 1);
    if constexpr (!WL) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int k4 = 0; k4 < KP / 4; ++k4)
                wv[q][k4] = *reinterpret_cast<const MST_GLOBAL_AS lstm_f4u*>(whh + min((q * H + uc) * H + 4 * k4, wlast));
        }
    }
    float bias[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) bias[q] = bhh[q * H + uc];
    // the zx rows of the zchunk steps from `step` on: lane j < G takes column j, NT (clamped) loads in flight per trip
    constexpr int NT = 16;                          // loads in flight per trip
    auto fetch = [&](const int step) {
        const int cnt = min(zchunk, d.S - step);
        if (u < G) {
            const int sstep = d.reverse ? -G : G;
            const MST_GLOBAL_AS float* zg = zx + (int64_t)(d.reverse ? d.S - 1 - step : step) * G + u;
            for (int i0 = 0; i0 < cnt; i0 += NT) {
                float t[NT];
#pragma unroll
                for (int i = 0; i < NT; ++i) t[i] = zg[(int64_t)min(i0 + i, cnt - 1) * sstep];
#pragma unroll
                for (int i = 0; i < NT; ++i) MST_PIN(t[i]);
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    if (i0 + i < cnt) zx_s[(i0 + i) * G + u] = t[i];
                }
            }
        }
    };
    fetch(0);                // behind the weight and bias loads: one memory round trip for all three
    x_s[u] = 0.f;            // LSTM_SW_X = one float per lane
    if constexpr (WL) lstm_small_stage_whh<KP, false>(whh, H, u, w_s);
#pragma unroll
    for (int q = 0; q < 4; ++q) MST_PIN(bias[q]);
    float w[WL ? 1 : 4][WL ? 1 : KP];
#pragma unroll
    for (int q = 0; q < (WL ? 0 : 4); ++q) {
#pragma unroll
        for (int k4 = 0; k4 < KP / 4; ++k4) {
            const int flat = (q * H + uc) * H + 4 * k4, sh = flat - min(flat, wlast);       // 0 but at the end of the matrix
            const lstm_f4u r = wv[q][k4];
            float v0 = r.x, v1 = r.y, v2 = r.z;
            v0 = sh == 1 ? r.y : v0; v0 = sh == 2 ? r.z : v0; v0 = sh == 3 ? r.w : v0;
            v1 = sh == 1 ? r.z : v1; v1 = sh == 2 ? r.w : v1;
            v2 = sh == 1 ? r.w : v2;
            w[q][4 * k4] = 4 * k4 < H ? v0 : 0.f; w[q][4 * k4 + 1] = 4 * k4 + 1 < H ? v1 : 0.f;
            w[q][4 * k4 + 2] = 4 * k4 + 2 < H ? v2 : 0.f; w[q][4 * k4 + 3] = 4 * k4 + 3 < H ? r.w : 0.f;
        }
    }
    float c = 0.f, hown = 0.f;
    int slot = 0;
    const int rstep = d.reverse ? -1 : 1;
    int64_t row = (int64_t)bi * d.S + (d.reverse ? d.S - 1 : 0);
    for (int step = 0; step < d.S; ++step, ++slot, row += rstep) {
        if (slot == zchunk) {                          // wave-uniform
            MST_WAVE_SYNC();                           // the gate lanes are done with the previous chunk
            fetch(step);
            slot = 0;
        }
        MST_WAVE_SYNC();                               // h_{t-1} and the staged rows are in the slice
        float hv[KP], zq[4];
#pragma unroll
        for (int k = 0; k < KP; ++k) hv[k] = x_s[k];
#pragma unroll
        for (int q = 0; q < 4; ++q) zq[q] = zx_s[slot * G + q * H + uc];
        MST_WAVE_SYNC();                               // every lane has read h_{t-1} before one writes h_t
        if (u < H) {
            float a[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float z[4] = {0.f, 0.f, 0.f, 0.f};     // 4 independent FMA chains, k ascending in each
                if constexpr (WL) {
                    float wq[KP];
#pragma unroll
                    for (int k = 0; k < KP; ++k) wq[k] = w_s[(q * KP + k) * KP + u];
#pragma unroll
                    for (int k = 0; k < KP; k += 4) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) z[r] = fmaf(wq[k + r], hv[k + r], z[r]);
                    }
                    __builtin_amdgcn_sched_barrier(0);      // one gate's weights at a time: the rider's register budget
                } else {
#pragma unroll
                    for (int k = 0; k < KP; k += 4) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) z[r] = fmaf(w[q][k + r], hv[k + r], z[r]);
                    }
                }
                a[q] = (((z[0] + z[1]) + (z[2] + z[3])) + zq[q]) + bias[q];
            }
            const float ig = sigm(a[0]), fg = sigm(a[1]), gg = tanh_fast(a[2]), og = sigm(a[3]);
            c = lstm_cell_update(fg, c, ig, gg);
            const float tc = tanh_fast(c);
            const float h = og * tc;
            x_s[u] = h;
            tmp[d.hprev_off + row * H + u] = hown;
            tmp[d.tc_off + row * H + u] = tc;
            MST_GLOBAL_AS float* g = tmp + d.gates_off + row * G;
            g[u] = ig; g[H + u] = fg; g[2 * H + u] = gg; g[3 * H + u] = og;
            tmp[d.c_off + row * H + u] = c;
            ws[d.out_off + row * d.out_ld + u] = h;
            hown = h;
        }
    }
}

template <int KP, bool WL = false>
__device__ __forceinline__ void lstm_small_bwd_body(const LstmDesc& d, const int bi, const int u, const Bases& b, float* lds) {
    const int H = d.H, G = 4 * d.H;
    float* dz_s = lds;                             // dz_t: part p at 16 p, zero beyond H
    float* w_s = lds + LSTM_SW_X;                  // WL: the weights
    float* sv_s = lds + LSTM_SW_X + (WL ? LSTM_WL_F(KP) : 0);      // the seven streamed operands of the next schunk steps
    const int schunk = (LSTM_SW_LDS - LSTM_SW_X - (WL ? LSTM_WL_F(KP) : 0)) / (7 * H);
    const MST_GLOBAL_AS float* whh = (const MST_GLOBAL_AS float*)(b.p[SP_PAR] + d.whh_off);
    const MST_GLOBAL_AS float* tmp = (const MST_GLOBAL_AS float*)b.p[SP_TMP];
    MST_GLOBAL_AS float* gr = (MST_GLOBAL_AS float*)b.p[SP_GRAD];
    const int uc = min(u, H - 1);
    // column u of every part: w[p][jj] = W_hh[p H + jj, u] (coalesced along u), zero beyond H
    float w[WL ? 1 : 4][WL ? 1 : KP];
#pragma unroll
    for (int p = 0; p < (WL ? 0 : 4); ++p) {
#pragma unroll
        for (int jj = 0; jj < KP; ++jj) {
            const float v = whh[(p * H + min(jj, H - 1)) * H + uc];
            w[p][jj] = jj < H ? v : 0.f;
        }
    }
    // saved gates, tanh(c_t), c_{t-1} and the incoming gradient of the schunk steps from `step` down: lane (lane / 16, lane % 16)
    // takes every fourth of them for unit lane % 16
    const int ku = u & 15, kq = u >> 4;
    auto stage = [&](const int step) {
        const int cnt = min(schunk, step + 1);
        if (ku < H) {
#pragma unroll(WL ? 2 : 4)
            for (int i = kq; i < cnt; i += 4) {         // independent loads, 28 in flight (the rider form: 14)
                const int st = step - i;
                const int s_ = d.reverse ? d.S - 1 - st : st, sp_ = d.reverse ? s_ + 1 : s_ - 1;
                const int64_t row_ = (int64_t)bi * d.S + s_;
                const MST_GLOBAL_AS float* g_ = tmp + d.gates_off + row_ * G;
                float t[7];
                t[0] = g_[ku]; t[1] = g_[H + ku]; t[2] = g_[2 * H + ku]; t[3] = g_[3 * H + ku];
                t[4] = tmp[d.tc_off + row_ * H + ku];
                const float cp = tmp[d.c_off + ((int64_t)bi * d.S + (st > 0 ? sp_ : s_)) * H + ku];      // unconditional (clamped)
                t[5] = st > 0 ? cp : 0.f;
                t[6] = gr[d.gout_off + row_ * d.out_ld + ku];
#pragma unroll
                for (int q = 0; q < 7; ++q) sv_s[(i * 7 + q) * H + ku] = t[q];
            }
        }
    };
    stage(d.S - 1);          // behind the weight loads: one memory round trip for both
    dz_s[u] = 0.f;           // LSTM_SW_X = one float per lane
    if constexpr (WL) lstm_small_stage_whh<KP, true>(whh, H, u, w_s);
#pragma unroll
    for (int p = 0; p < (WL ? 0 : 4); ++p) {
#pragma unroll
        for (int jj = 0; jj < KP; ++jj) MST_PIN(w[p][jj]);
    }
    float dc_next = 0.f, red[4] = {0.f, 0.f, 0.f, 0.f};
    int slot = 0;
    const int rstep = d.reverse ? 1 : -1;
    int64_t row = (int64_t)bi * d.S + (d.reverse ? 0 : d.S - 1);
    for (int step = d.S - 1; step >= 0; --step, ++slot, row += rstep) {
        if (slot == schunk) {                          // wave-uniform
            MST_WAVE_SYNC();                           // the gate lanes are done with the previous chunk
            stage(step);
            slot = 0;
        }
        MST_WAVE_SYNC();                               // the staged operands are in the slice; dz_{t+1} has been read by every lane
        if (u < H) {
            float sv[7];
#pragma unroll
            for (int q = 0; q < 7; ++q) sv[q] = sv_s[(slot * 7 + q) * H + u];
            const float ig = sv[0], fg = sv[1], gg = sv[2], og = sv[3], tc = sv[4], cprev = sv[5];
            const float dh = sv[6] + ((red[0] + red[1]) + (red[2] + red[3]));
            const float dc = LSTM_MULADD(dh * og, LSTM_MULADD(-tc, tc, 1.f), dc_next);      // dc_next + dh * og * (1 - tc * tc)
            const float dzi = dc * gg * ig * (1.f - ig);
            const float dzf = dc * cprev * fg * (1.f - fg);
            const float dzg = dc * ig * LSTM_MULADD(-gg, gg, 1.f);                          // dc * ig * (1 - gg * gg)
            const float dzo = dh * tc * og * (1.f - og);
            dc_next = dc * fg;
            dz_s[u] = dzi; dz_s[16 + u] = dzf; dz_s[32 + u] = dzg; dz_s[48 + u] = dzo;
            MST_GLOBAL_AS float* gz = gr + d.gzx_off + row * G;
            gz[u] = dzi; gz[H + u] = dzf; gz[2 * H + u] = dzg; gz[3 * H + u] = dzo;
        }
        if (step == 0) break;                          // dh_{-1} feeds nothing
        MST_WAVE_SYNC();                               // dz_t is in the slice
        // dh_{t-1}[u] = sum_j W_hh[j, u] dz_t[j]: per part four FMA chains, jj ascending in each; the parts are added by the next step
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float dv[KP];
#pragma unroll
            for (int jj = 0; jj < KP; ++jj) dv[jj] = dz_s[16 * p + jj];
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (WL) {
                float wp[KP];
#pragma unroll
                for (int jj = 0; jj < KP; ++jj) wp[jj] = w_s[(p * KP + jj) * KP + uc];
#pragma unroll
                for (int jj = 0; jj < KP; jj += 4) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) a[r] = fmaf(wp[jj + r], dv[jj + r], a[r]);
                }
                __builtin_amdgcn_sched_barrier(0);          // one part's weights at a time: the rider's register budget
            } else {
#pragma unroll
                for (int jj = 0; jj < KP; jj += 4) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) a[r] = fmaf(w[p][jj + r], dv[jj + r], a[r]);
                }
            }
            red[p] = (a[0] + a[1]) + (a[2] + a[3]);
        }
    }
}
