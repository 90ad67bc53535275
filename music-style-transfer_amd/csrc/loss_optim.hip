// get_total_loss (style/model.py:847-997), Adam+StepLR (train-model.py:89-90,151-154) and
// hard_output (style/model.py:818-832) for gfx950.
//
// Loss = one streaming reduction over predictions/targets (7 partial sums per note tensor,
// HBM-bound, coalesced, per-workgroup partials re-summed in order), a single-lane scalar tail
// tail that evaluates the reference's loss tree with forward-mode dual numbers (16 lanes, one
// per tape input) — so every data-dependent Python branch of the reference (safe_div, safe_sqrt)
// is taken on the device with identical values AND gradients, with no host sync — and one
// elementwise backward pass.  The tail yields the full Jacobian d(leaf)/d(partial sum), so any
// loss leaf can be differentiated.
#include "mst_common.h"

#define LOSS_MAXBLK 256
#define NP_SUMS 7            // TP FP FN SEvel SEdur BCE Nmask
#define N_TAPE_IN 16         // 7 pitched + 6 unpitched + instruments, mode, bpm raw losses
#define SAVED_J 0            // saved[k*16 + j] = d leaf_k / d input_j
#define EPS_DIV 1e-7f

int64_t mst_loss_scratch_floats(void) { return 2 * LOSS_MAXBLK * 8 + 64; }

// ------------------------------------------------------------------ streaming partial sums
template <int NFEAT>
__device__ __forceinline__ void note_terms(const float* p, const float* t, float* acc) {
    const float pv = p[1], tv = t[1];
    const float m = tv > 0.f ? 1.f : 0.f;
    acc[0] += fminf(pv, tv);
    acc[1] += fmaxf(pv - tv, 0.f);
    acc[2] += fmaxf(tv - pv, 0.f);
    const float dv = tv - pv;
    acc[3] += dv * dv * m;
    const float dd = (p[0] - fminf(t[0], 6.f)) / 6.f;
    acc[4] += dd * dd * m;
    if (NFEAT == 5) {
        float bce = 0.f;
#pragma unroll
        for (int a = 2; a < 5; ++a) {   // F.binary_cross_entropy clamps both logs at -100
            const float lp = fmaxf(logf(p[a]), -100.f), lq = fmaxf(logf(1.f - p[a]), -100.f);
            bce -= t[a] * lp + (1.f - t[a]) * lq;
        }
        acc[5] += bce * m;
    }
    acc[6] += m;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// grid (nblk_p + nblk_u): first nblk_p workgroups reduce the pitched tensor, the rest the unpitched
// blockIdx.y = clip of a batched plan (per-clip pointer strides in lb; all 0 for a single clip)
__global__ __launch_bounds__(256) void loss_partials_kernel(const float* pp, const float* pt, int64_t np, int nblk_p,
                                                            const float* up, const float* ut, int64_t nu, int nblk_u,
                                                            float* scratch, LossBatch lb) {
    __shared__ float red[4][NP_SUMS];
    __shared__ float tile_p[256 * 5], tile_t[256 * 5];
    {
        const int64_t k = blockIdx.y;
        pp += k * lb.ws; pt += k * lb.ext0; up += k * lb.ws; ut += k * lb.ext1; scratch += k * lb.tmp;
    }
    const bool pitched = (int)blockIdx.x < nblk_p;
    const int blk = pitched ? blockIdx.x : blockIdx.x - nblk_p;
    const int nb = pitched ? nblk_p : nblk_u;
    const int64_t n = pitched ? np : nu;
    float acc[NP_SUMS];
#pragma unroll
    for (int k = 0; k < NP_SUMS; ++k) acc[k] = 0.f;
    // a tile of 256 positions is staged through LDS with unit-stride loads (a lane's own 5-float record is a stride-5
    // access: every wave load touched 5 x the cache lines it used); lane <-> position and the order of a lane's sums are unchanged
    const int nf = pitched ? 5 : 2;
    const float* P = pitched ? pp : up;
    const float* T = pitched ? pt : ut;
    for (int64_t base = (int64_t)blk * 256; base < n; base += (int64_t)nb * 256) {
        const int rows = (int)(n - base < 256 ? n - base : 256), cnt = rows * nf;
        // global-address-space pointers: through generic ones every load waits for the previous LDS store (may alias)
        const MST_GLOBAL_AS float* Pg = (const MST_GLOBAL_AS float*)(P + base * nf);
        const MST_GLOBAL_AS float* Tg = (const MST_GLOBAL_AS float*)(T + base * nf);
        {
            float pv[5], tv[5];
#pragma unroll
            for (int u = 0; u < 5; ++u) {           // clamped, unconditional: all ten loads in flight
                const int j = min((int)threadIdx.x + 256 * u, cnt - 1);
                pv[u] = Pg[j]; tv[u] = Tg[j];
            }
#pragma unroll
            for (int u = 0; u < 5; ++u) {
                const int j = threadIdx.x + 256 * u;
                if (j < cnt) { tile_p[j] = pv[u]; tile_t[j] = tv[u]; }
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < rows) {
            if (pitched) note_terms<5>(tile_p + threadIdx.x * 5, tile_t + threadIdx.x * 5, acc);
            else note_terms<2>(tile_p + threadIdx.x * 2, tile_t + threadIdx.x * 2, acc);
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < NP_SUMS; ++k) acc[k] = wave_sum(acc[k]);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NP_SUMS; ++k) red[wv][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < NP_SUMS) {
        const int k = threadIdx.x;
        float* dst = scratch + (pitched ? 0 : LOSS_MAXBLK * 8);
        dst[blk * 8 + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    }
}

// ------------------------------------------------------------------ scalar tail, forward-mode AD
// The reference's loss tree (style/model.py:847-997) evaluated with dual numbers: lane j (< 16)
// carries d/d(input_j), so one pass over ~100 scalar ops yields every loss leaf AND the full
// Jacobian d(leaf)/d(partial sum) — all in registers, no tape.  The reference's data-dependent
// Python branches (safe_div, safe_sqrt) become value-dependent selects with identical values
// and gradients.
struct Dual { float v, d; };
__device__ __forceinline__ Dual dl(float v, float d) { Dual r; r.v = v; r.d = d; return r; }
__device__ __forceinline__ Dual d_add(Dual a, Dual b) { return dl(a.v + b.v, a.d + b.d); }
__device__ __forceinline__ Dual d_mul(Dual a, Dual b) { return dl(a.v * b.v, a.d * b.v + a.v * b.d); }
__device__ __forceinline__ Dual d_cmul(Dual a, float c) { return dl(a.v * c, a.d * c); }
__device__ __forceinline__ Dual d_one_minus(Dual a) { return dl(1.f - a.v, -a.d); }
__device__ __forceinline__ Dual d_sqr(Dual a) { return dl(a.v * a.v, 2.f * a.v * a.d); }
__device__ __forceinline__ Dual d_div(Dual a, Dual b) { const float q = a.v / b.v; return dl(q, (a.d - q * b.d) / b.v); }
__device__ __forceinline__ Dual d_safe_div(Dual a, Dual b) {          // style/model.py:854-860
    float den = b.v;
    if (fabsf(den) < EPS_DIV) den = den < 0.f ? den - EPS_DIV : den + EPS_DIV;
    const float q = a.v / den;
    return dl(q, (a.d - q * b.d) / den);
}
__device__ __forceinline__ Dual d_safe_sqrt(Dual a) {                  // style/utils/pytorch.py:68-71
    if (a.v == 0.f) return dl(0.f, 0.f);
    const float r = sqrtf(a.v);
    return dl(r, a.d * 0.5f / r);
}
__device__ __forceinline__ Dual d_tanh(Dual a) { const float t = tanhf(a.v); return dl(t, a.d * (1.f - t * t)); }
// quadratic mean with constant weights 1/k (get_mean, style/utils/pytorch.py:74-94)
__device__ __forceinline__ Dual d_qmean2(Dual a, Dual b) { return d_safe_sqrt(d_add(d_cmul(d_sqr(a), 0.5f), d_cmul(d_sqr(b), 0.5f))); }
__device__ __forceinline__ Dual d_qmean3(Dual a, Dual b, Dual c) {
    const float w = (float)(1.0 / 3.0);
    return d_safe_sqrt(d_add(d_add(d_cmul(d_sqr(a), w), d_cmul(d_sqr(b), w)), d_cmul(d_sqr(c), w)));
}

struct ChannelLeaves { Dual total, notes, vel, dur, acc; };

// channels losses of one note tensor from its partial sums (style/model.py:863-932)
__device__ __forceinline__ ChannelLeaves channel_tree(const Dual* in, bool pitched, bool normalize) {
    const Dual TP = in[0], FP = in[1], FN = in[2], SEV = in[3], SED = in[4];
    const Dual NM = pitched ? in[6] : in[5];
    ChannelLeaves o;
    const Dual prec = d_safe_div(TP, d_add(TP, FP));
    const Dual rec = d_safe_div(TP, d_add(TP, FN));
    const Dual f = d_cmul(d_safe_div(d_mul(prec, rec), d_add(prec, rec)), 2.f);
    o.notes = d_one_minus(f);
    o.vel = d_div(SEV, NM);
    o.dur = d_div(SED, NM);
    // first learn the right notes, then the right velocities: weights [notes, 1 - notes] are live
    const Dual nv = d_safe_sqrt(d_add(d_mul(o.notes, d_sqr(o.notes)), d_mul(d_one_minus(o.notes), d_sqr(o.vel))));
    if (pitched) {
        o.acc = d_div(in[5], d_cmul(NM, 3.f));
        if (normalize) o.acc = d_tanh(o.acc);
        o.total = d_qmean3(o.dur, o.acc, nv);
    } else {
        o.acc = dl(0.f, 0.f);
        o.total = d_qmean2(o.dur, nv);
    }
    return o;
}

__global__ __launch_bounds__(64) void loss_tail_kernel(const float* scratch, int nblk_p, int nblk_u, int has_u,
                                                       const float* il, const float* it, int ni,
                                                       const float* mlg, const float* mt,
                                                       const float* bp, const float* bt, int normalize,
                                                       float* losses, float* saved, LossBatch lb,
                                                       float* gl_onehot, float* losses_out) {
    __shared__ float sums[N_TAPE_IN];
    const int tid = threadIdx.x;
    {
        const int64_t k = blockIdx.y;
        scratch += k * lb.tmp; il += k * lb.ws; it += k * lb.ws; mlg += k * lb.ws; mt += k * lb.ws; bp += k * lb.ws;
        bt += k * lb.ws; losses += k * lb.ws; saved += k * lb.ws;
        // train-iteration extras (null for the stand-alone entry point): the upstream gradient of loss.backward() — one-hot
        // on the total — and a dense copy of the leaves for the caller, written here instead of by two more launches
        if (gl_onehot) gl_onehot += k * lb.ws;
        if (losses_out) losses_out += k * MST_N_LOSSES;
    }
    // partial rows hold 7 sums {TP FP FN SEvel SEdur BCE Nmask}; tape inputs 0..6 are the pitched tensor's,
    // 7..12 the unpitched tensor's {TP FP FN SEvel SEdur Nmask}.  Lanes stride over the per-workgroup partials,
    // then a fixed-order wave reduction (the tail is one 64-lane wave).
    // A lane takes whole 8-float partial rows (two 16-byte loads per row, both tensors' loops in flight together) instead of
    // fourteen dependent strided passes; per lane and per sum the order over q, and the wave reduction, are the same.
    {
        float sp[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, su[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        typedef float row4 __attribute__((ext_vector_type(4), aligned(4)));      // 16-byte load, 4-byte alignment suffices
        const row4* rp = reinterpret_cast<const row4*>(scratch);
        const row4* ru = reinterpret_cast<const row4*>(scratch + LOSS_MAXBLK * 8);
        const int nbu = has_u ? nblk_u : 0;
        for (int q = tid; q < nblk_p; q += 64) {
            const row4 x = rp[2 * q], y = rp[2 * q + 1];
            sp[0] += x.x; sp[1] += x.y; sp[2] += x.z; sp[3] += x.w; sp[4] += y.x; sp[5] += y.y; sp[6] += y.z;
        }
        for (int q = tid; q < nbu; q += 64) {
            const row4 x = ru[2 * q], y = ru[2 * q + 1];
            su[0] += x.x; su[1] += x.y; su[2] += x.z; su[3] += x.w; su[4] += y.x; su[5] += y.y; su[6] += y.z;
        }
#pragma unroll
        for (int k = 0; k < 7; ++k) { sp[k] = wave_sum(sp[k]); su[k] = wave_sum(su[k]); }
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < 7; ++k) sums[k] = sp[k];
#pragma unroll
            for (int k = 0; k < 5; ++k) sums[7 + k] = su[k];
            sums[12] = su[6];
        }
    }
    // instruments: BCE-with-logits, mean over ni (style/model.py:903)
    float v = 0.f;
    for (int j = tid; j < ni; j += 64) {
        const float x = il[j];
        v += fmaxf(x, 0.f) - x * it[j] + log1pf(expf(-fabsf(x)));
    }
    v = wave_sum(v);
    if (tid == 0) {
        sums[13] = v / (float)ni;
        // mode: cross entropy against argmax of the one-hot target (style/model.py:904), 2 classes
        const int tgt = mt[1] > mt[0] ? 1 : 0;
        const float mx = fmaxf(mlg[0], mlg[1]);
        const float lse = mx + logf(expf(mlg[0] - mx) + expf(mlg[1] - mx));
        sums[14] = lse - mlg[tgt];
        const float db = (bp[0] - bt[0]) / 150.f;
        sums[15] = db * db;
    }
    __syncthreads();
    if (tid >= N_TAPE_IN) return;
    Dual in[N_TAPE_IN];
#pragma unroll
    for (int j = 0; j < N_TAPE_IN; ++j) in[j] = dl(sums[j], j == tid ? 1.f : 0.f);
    Dual leaf[MST_N_LOSSES];
    bool present[MST_N_LOSSES];
#pragma unroll
    for (int k = 0; k < MST_N_LOSSES; ++k) { leaf[k] = dl(0.f, 0.f); present[k] = true; }
    const ChannelLeaves p = channel_tree(in, true, normalize != 0);
    leaf[MST_L_P_TOTAL] = p.total; leaf[MST_L_P_NOTES] = p.notes; leaf[MST_L_P_VELOCITY] = p.vel;
    leaf[MST_L_P_DURATION] = p.dur; leaf[MST_L_P_ACCIDENTALS] = p.acc;
    if (has_u) {
        const ChannelLeaves u = channel_tree(in + 7, false, normalize != 0);
        leaf[MST_L_U_TOTAL] = u.total; leaf[MST_L_U_NOTES] = u.notes; leaf[MST_L_U_VELOCITY] = u.vel;
        leaf[MST_L_U_DURATION] = u.dur;
        leaf[MST_L_CH_TOTAL] = d_qmean2(p.total, u.total);
    } else {
        present[MST_L_U_TOTAL] = present[MST_L_U_NOTES] = present[MST_L_U_VELOCITY] = present[MST_L_U_DURATION] = false;
        leaf[MST_L_CH_TOTAL] = p.total;
    }
    Dual li = in[13], lm = in[14];
    if (normalize) { li = d_tanh(li); lm = d_tanh(lm); }
    leaf[MST_L_SI_INSTRUMENTS] = li;
    leaf[MST_L_SI_MODE] = lm;
    leaf[MST_L_SI_BPM] = in[15];
    leaf[MST_L_SI_TOTAL] = d_qmean3(li, lm, in[15]);
    leaf[MST_L_TOTAL] = d_qmean2(leaf[MST_L_CH_TOTAL], leaf[MST_L_SI_TOTAL]);
#pragma unroll
    for (int k = 0; k < MST_N_LOSSES; ++k) {
        if (tid == 0) {
            const float v = present[k] ? leaf[k].v : __builtin_nanf("");
            losses[k] = v;
            if (losses_out) losses_out[k] = v;
            if (gl_onehot) gl_onehot[k] = k == MST_L_TOTAL ? 1.f : 0.f;
        }
        saved[SAVED_J + k * N_TAPE_IN + tid] = present[k] ? leaf[k].d : 0.f;
    }
}

// ------------------------------------------------------------------ elementwise backward
// grid (nblk_p + nblk_u + 1): note-tensor gradients, last workgroup = song-info head gradients
__global__ __launch_bounds__(256) void loss_bwd_kernel(const float* pp, const float* pt, int64_t np, int nblk_p,
                                                       const float* up, const float* ut, int64_t nu, int nblk_u,
                                                       const float* il, const float* it, int ni,
                                                       const float* mlg, const float* mt, const float* bp, const float* bt,
                                                       const float* saved, const float* gl,
                                                       float* gp, float* gu, float* gi, float* gm, float* gb, LossBatch lb, float info_scale) {
    __shared__ float coef[N_TAPE_IN];
    __shared__ float tile_p[256 * 5], tile_t[256 * 5];
    {
        const int64_t k = blockIdx.y;
        pp += k * lb.ws; pt += k * lb.ext0; up += k * lb.ws; ut += k * lb.ext1;
        il += k * lb.ws; it += k * lb.ws; mlg += k * lb.ws; mt += k * lb.ws; bp += k * lb.ws; bt += k * lb.ws;
        saved += k * lb.ws; gl += k * lb.ws;
        gp += k * lb.grad; gu += k * lb.grad; gi += k * lb.grad; gm += k * lb.grad; gb += k * lb.grad;
    }
    if (threadIdx.x < N_TAPE_IN) {
        // all 30 loads first (a conditional load per leaf was a chain of 15 dependent round trips at the head of every workgroup)
        float gk[MST_N_LOSSES], sk[MST_N_LOSSES];
#pragma unroll
        for (int k = 0; k < MST_N_LOSSES; ++k) { gk[k] = gl[k]; sk[k] = saved[SAVED_J + k * N_TAPE_IN + threadIdx.x]; }
        float c = 0.f;
#pragma unroll
        for (int k = 0; k < MST_N_LOSSES; ++k) c += gk[k] != 0.f ? gk[k] * sk[k] : 0.f;
        coef[threadIdx.x] = c;
    }
    __syncthreads();
    const int bx = blockIdx.x;
    if (bx < nblk_p + nblk_u) {
        const bool pitched = bx < nblk_p;
        const int blk = pitched ? bx : bx - nblk_p;
        const int nb = pitched ? nblk_p : nblk_u;
        const int64_t n = pitched ? np : nu;
        const int nf = pitched ? 5 : 2;
        const float* P = pitched ? pp : up;
        const float* T = pitched ? pt : ut;
        float* G = pitched ? gp : gu;
        const float* c = coef + (pitched ? 0 : 7);
        const float cTP = c[0], cFP = c[1], cFN = c[2], cSEV = c[3], cSED = c[4];
        const float cBCE = pitched ? c[5] : 0.f;
        // tiles of 256 positions through LDS: unit-stride loads and stores (see loss_partials_kernel)
        for (int64_t base = (int64_t)blk * 256; base < n; base += (int64_t)nb * 256) {
            const int rows = (int)(n - base < 256 ? n - base : 256), cnt = rows * nf;
            const MST_GLOBAL_AS float* Pg = (const MST_GLOBAL_AS float*)(P + base * nf);
            const MST_GLOBAL_AS float* Tg = (const MST_GLOBAL_AS float*)(T + base * nf);
            MST_GLOBAL_AS float* Gg = (MST_GLOBAL_AS float*)(G + base * nf);
            {
                float pv[5], tv[5];
#pragma unroll
                for (int u = 0; u < 5; ++u) {       // clamped, unconditional: all ten loads in flight
                    const int j = min((int)threadIdx.x + 256 * u, cnt - 1);
                    pv[u] = Pg[j]; tv[u] = Tg[j];
                }
#pragma unroll
                for (int u = 0; u < 5; ++u) {
                    const int j = threadIdx.x + 256 * u;
                    if (j < cnt) { tile_p[j] = pv[u]; tile_t[j] = tv[u]; }
                }
            }
            __syncthreads();
            if ((int)threadIdx.x < rows) {
                float* p = tile_p + threadIdx.x * nf;             // the gradient record replaces the prediction's
                const float* t = tile_t + threadIdx.x * nf;
                const float pv = p[1], tv = t[1], p0 = p[0];
                const float m = tv > 0.f ? 1.f : 0.f;
                // torch.min splits the gradient on ties; relu'(0) = 0
                float gv = cTP * (pv < tv ? 1.f : (pv == tv ? 0.5f : 0.f));
                gv += cFP * (pv - tv > 0.f ? 1.f : 0.f) - cFN * (tv - pv > 0.f ? 1.f : 0.f);
                gv -= cSEV * 2.f * (tv - pv) * m;
                p[1] = gv;
                p[0] = cSED * 2.f * (p0 - fminf(t[0], 6.f)) * (1.f / 36.f) * m;
                if (pitched) {
#pragma unroll
                    for (int a = 2; a < 5; ++a)   // aten binary_cross_entropy_backward
                        p[a] = cBCE * m * (p[a] - t[a]) / fmaxf((1.f - p[a]) * p[a], 1e-12f);
                }
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 5; ++u) {
                const int j = threadIdx.x + 256 * u;
                if (j < cnt) Gg[j] = tile_p[j];
            }
            __syncthreads();
        }
    } else {
        const float ci = coef[13] * info_scale, cm = coef[14] * info_scale, cb = coef[15] * info_scale;
        // d tanh already folded into coef (the tape's inputs are the raw losses)
        for (int j = threadIdx.x; j < ni; j += 256) gi[j] = ci * (1.f / (1.f + expf(-il[j])) - it[j]) / (float)ni;
        if (threadIdx.x == 0) {
            const int tgt = mt[1] > mt[0] ? 1 : 0;
            const float mx = fmaxf(mlg[0], mlg[1]);
            const float e0 = expf(mlg[0] - mx), e1 = expf(mlg[1] - mx);
            gm[0] = cm * (e0 / (e0 + e1) - (tgt == 0 ? 1.f : 0.f));
            gm[1] = cm * (e1 / (e0 + e1) - (tgt == 1 ? 1.f : 0.f));
            gb[0] = cb * 2.f * (bp[0] - bt[0]) / (150.f * 150.f);
        }
    }
}

static int blocks_for(int64_t n) {
    int64_t b = (n + 1023) / 1024;
    if (b < 1) b = 1;
    if (b > LOSS_MAXBLK) b = LOSS_MAXBLK;
    return (int)b;
}

int loss_fwd_batched(const float* pp, const float* pt, int64_t np, const float* up, const float* ut, int64_t nu, const float* il,
                     const float* it, int ni, const float* mlg, const float* mt, const float* bp, const float* bt, int normalize,
                     float* losses, float* saved, float* scratch, LossBatch lb, hipStream_t s, float* gl_onehot, float* losses_out) {
    if (!pp || !pt || !il || !it || !mlg || !mt || !bp || !bt || !losses || !saved || !scratch || np <= 0 || lb.clips < 1)
        return MST_ERR_ARG;
    const int has_u = (up && ut && nu > 0) ? 1 : 0;
    const int nbp = blocks_for(np), nbu = has_u ? blocks_for(nu) : 0;
    hipLaunchKernelGGL(loss_partials_kernel, dim3(nbp + nbu, lb.clips), dim3(256), 0, s, pp, pt, np, nbp, up, ut,
                       has_u ? nu : (int64_t)0, nbu, scratch, lb);
    hipLaunchKernelGGL(loss_tail_kernel, dim3(1, lb.clips), dim3(64), 0, s, (const float*)scratch, nbp, nbu, has_u, il, it,
                       ni, mlg, mt, bp, bt, normalize, losses, saved, lb, gl_onehot, losses_out);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

int loss_bwd_batched(const float* pp, const float* pt, int64_t np, const float* up, const float* ut, int64_t nu, const float* il,
                     const float* it, int ni, const float* mlg, const float* mt, const float* bp, const float* bt,
                     const float* saved, const float* gl, float* gp, float* gu, float* gi, float* gm, float* gb, LossBatch lb,
                     hipStream_t s, float info_scale) {
    if (!pp || !pt || !saved || !gl || !gi || !gm || !gb || np <= 0 || lb.clips < 1) return MST_ERR_ARG;
    const int has_u = (up && ut && gu && nu > 0) ? 1 : 0;
    // gp == nullptr: the pitched tensor's gradient is not wanted here (the applier's backward kernel computes it on the fly)
    const int nbp = gp ? blocks_for(np) : 0, nbu = has_u ? blocks_for(nu) : 0;
    hipLaunchKernelGGL(loss_bwd_kernel, dim3(nbp + nbu + 1, lb.clips), dim3(256), 0, s, pp, pt, np, nbp, up, ut,
                       has_u ? nu : (int64_t)0, nbu, il, it, ni, mlg, mt, bp, bt, saved, gl, gp, gu, gi, gm, gb, lb, info_scale);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

static const LossBatch ONE_CLIP = {1, 0, 0, 0, 0, 0};

int loss_blocks(int64_t n) { return blocks_for(n); }

int loss_fwd_partials(const float* pp, const float* pt, int64_t np, const float* up, const float* ut, int64_t nu, float* scratch,
                      hipStream_t s) {
    const int has_u = (up && ut && nu > 0) ? 1 : 0;
    const int nbp = blocks_for(np), nbu = has_u ? blocks_for(nu) : 0;
    hipLaunchKernelGGL(loss_partials_kernel, dim3(nbp + nbu, 1), dim3(256), 0, s, pp, pt, np, nbp, up, ut,
                       has_u ? nu : (int64_t)0, nbu, scratch, ONE_CLIP);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

int loss_fwd_tail(int64_t np, int64_t nu, int has_u, const float* il, const float* it, int ni, const float* mlg, const float* mt,
                  const float* bp, const float* bt, int normalize, float* losses, float* saved, float* scratch, hipStream_t s,
                  float* gl_onehot, float* losses_out) {
    const int nbp = blocks_for(np), nbu = has_u ? blocks_for(nu) : 0;
    hipLaunchKernelGGL(loss_tail_kernel, dim3(1, 1), dim3(64), 0, s, (const float*)scratch, nbp, nbu, has_u, il, it,
                       ni, mlg, mt, bp, bt, normalize, losses, saved, ONE_CLIP, gl_onehot, losses_out);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

extern "C" int32_t mst_total_loss_fwd(const float* pp, const float* pt, int64_t np, const float* up, const float* ut,
                                      int64_t nu, const float* il, const float* it, int32_t ni, const float* mlg,
                                      const float* mt, const float* bp, const float* bt, int32_t normalize,
                                      float* losses, float* saved, float* scratch, mst_stream stream) {
    return loss_fwd_batched(pp, pt, np, up, ut, nu, il, it, (int)ni, mlg, mt, bp, bt, (int)normalize, losses, saved, scratch,
                            ONE_CLIP, (hipStream_t)stream, nullptr, nullptr);
}

extern "C" int32_t mst_total_loss_bwd(const float* pp, const float* pt, int64_t np, const float* up, const float* ut,
                                      int64_t nu, const float* il, const float* it, int32_t ni, const float* mlg,
                                      const float* mt, const float* bp, const float* bt, const float* saved,
                                      const float* gl, float* gp, float* gu, float* gi, float* gm, float* gb,
                                      mst_stream stream) {
    return loss_bwd_batched(pp, pt, np, up, ut, nu, il, it, (int)ni, mlg, mt, bp, bt, saved, gl, gp, gu, gi, gm, gb, ONE_CLIP,
                            (hipStream_t)stream);
}

// ------------------------------------------------------------------ Adam + StepLR
// state[0] = optimizer steps taken so far (t); the prepare kernel turns it into the step's
// scalars in double precision exactly as torch's Python-side arithmetic does, then bumps t.
__device__ __forceinline__ void adam_advance(float* state, double lr0, double b1, double b2, int step_size, double gamma) {
    const int t = (int)state[0] + 1;
    const double lr = lr0 * pow(gamma, (double)((t - 1) / step_size));
    const double bc1 = 1.0 - pow(b1, (double)t);
    const double bc2 = 1.0 - pow(b2, (double)t);
    state[0] = (float)t;
    state[1] = (float)(lr / bc1);
    state[2] = (float)sqrt(bc2);
}

__global__ void adam_prepare_kernel(float* state, double lr0, double b1, double b2, int step_size, double gamma) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    adam_advance(state, lr0, b1, b2, step_size, gamma);
}

// a * b rounded to fp32 on its own: hipcc contracts a product into a following add or subtract by default (and its __fmul_rn is
// a plain product), so the product is formed with contraction off and then made opaque
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
    float r = a * b;
    MST_PIN(r);
    return r;
}

// GUARD: the effective gradient is scaled by the guard record's coefficient first — "clip, then the same step"
template <bool GUARD>
__device__ __forceinline__ void adam_update(float* __restrict__ p, float* __restrict__ g, float* __restrict__ g2,
                                            float* __restrict__ m, float* __restrict__ v, int64_t n,
                                            const float* __restrict__ state, float b1, float b2, float eps, int zero_grad, float coef) {
    const float step = state[1], bc2s = state[2];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        // g2: gradients of a second, concurrently run accumulation iteration (same sum as accumulating in place)
        float gi = g2 ? g[i] + g2[i] : g[i];
        if (GUARD) gi = mul_rounded(gi, coef);
        const float mi = m[i] + (gi - m[i]) * (1.f - b1);        // exp_avg.lerp_(grad, 1 - beta1)
        const float vi = v[i] * b2 + (1.f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] -= step * (mi / (sqrtf(vi) / bc2s + eps));
        if (zero_grad) { g[i] = 0.f; if (g2) g2[i] = 0.f; }
    }
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ g2,
                                                   float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                   const float* __restrict__ state, float b1, float b2, float eps, int zero_grad) {
    adam_update<false>(p, g, g2, m, v, n, state, b1, b2, eps, zero_grad, 1.f);
}

static int32_t adam_launch(float* params, float* grads, float* grads2, float* exp_avg, float* exp_avg_sq, int64_t n, float* state,
                           double lr0, double beta1, double beta2, double eps, int32_t step_size, double gamma,
                           int32_t zero_grad, mst_stream stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !state || n <= 0 || step_size <= 0) return MST_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(adam_prepare_kernel, dim3(1), dim3(64), 0, s, state, lr0, beta1, beta2, (int)step_size, gamma);
    int64_t nb = (n + 1023) / 1024;
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)nb), dim3(256), 0, s, params, grads, grads2, exp_avg, exp_avg_sq, n,
                       (const float*)state, (float)beta1, (float)beta2, (float)eps, (int)zero_grad);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

extern "C" int32_t mst_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float* state,
                                 double lr0, double beta1, double beta2, double eps, int32_t step_size, double gamma,
                                 int32_t zero_grad, mst_stream stream) {
    return adam_launch(params, grads, nullptr, exp_avg, exp_avg_sq, n, state, lr0, beta1, beta2, eps, step_size, gamma, zero_grad, stream);
}

extern "C" int32_t mst_adam_step2(float* params, float* grads, float* grads2, float* exp_avg, float* exp_avg_sq, int64_t n,
                                  float* state, double lr0, double beta1, double beta2, double eps, int32_t step_size,
                                  double gamma, int32_t zero_grad, mst_stream stream) {
    if (!grads2) return MST_ERR_ARG;
    return adam_launch(params, grads, grads2, exp_avg, exp_avg_sq, n, state, lr0, beta1, beta2, eps, step_size, gamma, zero_grad, stream);
}

// ------------------------------------------------------------------ guarded step (mst_adam_step_guarded, mst_grad_norm, mst_grad_norms)
// Global-norm clipping and the skip of a non-finite step, decided on the device.  The flat gradient (g, or g + g2 formed in
// fp32 as adam_update forms it) is cut into slices of GS_SLICE elements, one workgroup and one double partial each: the number
// of partials depends on n alone, never on the device, and they are summed by one workgroup in a fixed order — no atomics, no
// workgroup waiting for another, the same bits on every run and every device.  The squares of fp32 values are exact in double
// (48 significant bits), so contracting square and add into an FMA changes nothing.
#define GS_SLICE 4096            // elements per workgroup: four 16-byte loads per lane and buffer
#define GS_THREADS 256
#define GS_WAVES (GS_THREADS / 64)
typedef float gs_f4 __attribute__((ext_vector_type(4)));

extern "C" int64_t mst_grad_guard_scratch_bytes(int64_t n) {
    if (n <= 0) return MST_ERR_ARG;
    return (n + GS_SLICE - 1) / GS_SLICE * (int64_t)sizeof(double);
}

// shuffles move 32 bits: a double travels as its two halves
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        unsigned w[2];
        __builtin_memcpy(w, &v, 8);
        w[0] = __shfl_xor(w[0], o);
        w[1] = __shfl_xor(w[1], o);
        double t;
        __builtin_memcpy(&t, w, 8);
        v += t;
    }
    return v;
}

// per-lane values -> wave sums -> the four wave sums through LDS, added in wave order; the total is valid in thread 0
__device__ __forceinline__ double gs_block_sum(double acc, double* red) {
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    double total = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < GS_WAVES; ++w) total += red[w];
    return total;
}

__device__ __forceinline__ double gs_sq4(double acc, gs_f4 x) {
    acc += (double)x.x * (double)x.x;
    acc += (double)x.y * (double)x.y;
    acc += (double)x.z * (double)x.z;
    acc += (double)x.w * (double)x.w;
    return acc;
}

// Workgroup b owns elements [b GS_SLICE, (b + 1) GS_SLICE) of the buffer.  s = element index + shift, shift = floats between the
// previous 16-byte boundary and g, so that s = 0 (mod 4) is a 16-byte-aligned address whatever the alignment of g; a group of
// four that is not wholly inside the slice (the ragged head and tail of a buffer that is only float-aligned) takes scalar loads.
// vec = 0: g2 sits at another 16-byte phase than g, every group takes scalar loads.  Lane l takes the groups l, l + 256, ... in
// order whichever path loads them.
__global__ __launch_bounds__(GS_THREADS) void grad_sumsq_kernel(const float* g, const float* g2, int64_t n, int shift, int vec,
                                                                double* partials) {
    __shared__ double red[GS_WAVES];
    const MST_GLOBAL_AS float* a = (const MST_GLOBAL_AS float*)g;
    const MST_GLOBAL_AS float* b = (const MST_GLOBAL_AS float*)g2;
    const int tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * GS_SLICE;
    const int64_t e1 = n - e0 < GS_SLICE ? n : e0 + GS_SLICE;
    double acc = 0.0;
    if (vec && shift == 0 && e1 - e0 == GS_SLICE) {                 // a whole, aligned slice: all loads in flight
        gs_f4 x[GS_SLICE / 4 / GS_THREADS];
#pragma unroll
        for (int u = 0; u < GS_SLICE / 4 / GS_THREADS; ++u)
            x[u] = *reinterpret_cast<const MST_GLOBAL_AS gs_f4*>(a + e0 + 4 * (tid + GS_THREADS * u));
        if (b) {
#pragma unroll
            for (int u = 0; u < GS_SLICE / 4 / GS_THREADS; ++u)
                x[u] += *reinterpret_cast<const MST_GLOBAL_AS gs_f4*>(b + e0 + 4 * (tid + GS_THREADS * u));
        }
#pragma unroll
        for (int u = 0; u < GS_SLICE / 4 / GS_THREADS; ++u) acc = gs_sq4(acc, x[u]);
    } else {
        const int64_t s0 = e0 + shift, s1 = e1 + shift;
        for (int i = tid; i < GS_SLICE / 4 + 1; i += GS_THREADS) {
            const int64_t s = e0 + 4 * i;
            if (vec && s >= s0 && s + 4 <= s1) {
                gs_f4 x = *reinterpret_cast<const MST_GLOBAL_AS gs_f4*>(a + (s - shift));
                if (b) x += *reinterpret_cast<const MST_GLOBAL_AS gs_f4*>(b + (s - shift));
                acc = gs_sq4(acc, x);
            } else {
                for (int j = 0; j < 4; ++j) {
                    if (s + j >= s0 && s + j < s1) {
                        const float ge = b ? a[s + j - shift] + b[s + j - shift] : a[s + j - shift];
                        acc += (double)ge * (double)ge;
                    }
                }
            }
        }
    }
    const double total = gs_block_sum(acc, red);
    if (tid == 0) partials[blockIdx.x] = total;
}

// one workgroup: the partials in a fixed order (per-lane chains over q = lane, lane + 256, ..., then gs_block_sum)
__device__ __forceinline__ double gs_total(const double* partials, int64_t np, double* red) {
    double acc = 0.0;
    for (int64_t q = threadIdx.x; q < np; q += GS_THREADS) acc += partials[q];
    return gs_block_sum(acc, red);
}

__global__ __launch_bounds__(GS_THREADS) void grad_norm_final_kernel(const double* partials, int64_t np, float* norm) {
    __shared__ double red[GS_WAVES];
    const double s = gs_total(partials, np, red);
    if (threadIdx.x == 0) norm[0] = (float)sqrt(s);
}

// adam_prepare_kernel of the guarded step: norm, coefficient and the skip decision into the guard record; the step counter
// and the step's scalars advance only when the step is taken
__global__ __launch_bounds__(GS_THREADS) void adam_prepare_guarded_kernel(float* state, float* guard, const double* partials, int64_t np,
                                                                          double lr0, double b1, double b2, int step_size, double gamma,
                                                                          float max_norm, int clip, int skip_nonfinite) {
    __shared__ double red[GS_WAVES];
    const double s = gs_total(partials, np, red);
    if (threadIdx.x != 0) return;
    const float norm = (float)sqrt(s);
    const bool nonfinite = (__float_as_uint(norm) & 0x7f800000u) == 0x7f800000u;      // inf or NaN, tested on the fp32 norm
    float coef = 1.f;
    if (clip && !nonfinite) {
        // torch.nn.utils.clip_grad_norm_: max_norm / (total_norm + 1e-6) clamped at 1, in the order torch evaluates it — a Python
        // float divided by a tensor is the tensor's reciprocal times the float, two fp32 roundings (one division is 1 ulp off at
        // g = [3, 4], max_norm = 2.5)
        const float c = max_norm * (1.f / (norm + 1e-6f));
        if (c < 1.f) coef = c;
    }
    const bool skip = skip_nonfinite && nonfinite;
    guard[0] = norm;
    guard[1] = skip ? 0.f : coef;
    guard[2] = skip ? 1.f : 0.f;
    if (skip) guard[3] += 1.f;
    if (coef < 1.f) guard[4] += 1.f;
    if (!nonfinite && norm > guard[5]) guard[5] = norm;
    guard[6] = guard[7] = 0.f;
    if (!skip) adam_advance(state, lr0, b1, b2, step_size, gamma);
}

__global__ __launch_bounds__(256) void adam_guarded_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ g2,
                                                           float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                           const float* __restrict__ state, const float* __restrict__ guard, float b1,
                                                           float b2, float eps, int zero_grad) {
    if (guard[2] != 0.f) {                          // skipped: p, m, v untouched; the bad gradient is still dropped
        if (zero_grad)
            for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
                g[i] = 0.f;
                if (g2) g2[i] = 0.f;
            }
        return;
    }
    adam_update<true>(p, g, g2, m, v, n, state, b1, b2, eps, zero_grad, guard[1]);
}

// one workgroup per tensor: per-lane chains over i = lane, lane + 256, ... in double, then gs_block_sum
__global__ __launch_bounds__(GS_THREADS) void grad_norms_kernel(const float* g, const float* g2, const int64_t* offsets,
                                                                const int64_t* lengths, float* norms) {
    __shared__ double red[GS_WAVES];
    const int64_t off = offsets[blockIdx.x], len = lengths[blockIdx.x];
    const MST_GLOBAL_AS float* a = (const MST_GLOBAL_AS float*)g + off;
    const MST_GLOBAL_AS float* b = g2 ? (const MST_GLOBAL_AS float*)g2 + off : nullptr;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < len; i += GS_THREADS) {
        const float ge = b ? a[i] + b[i] : a[i];
        acc += (double)ge * (double)ge;
    }
    const double total = gs_block_sum(acc, red);
    if (threadIdx.x == 0) norms[blockIdx.x] = (float)sqrt(total);
}

// enqueues grad_sumsq_kernel over the flat buffer; returns the number of partials, or a negative status
static int64_t gs_launch_sumsq(const float* grads, const float* grads2, int64_t n, void* scratch, hipStream_t s) {
    if (!grads || !scratch || n <= 0 || ((uintptr_t)scratch & 7) || ((uintptr_t)grads & 3) || ((uintptr_t)grads2 & 3)) return MST_ERR_ARG;
    const int64_t np = (n + GS_SLICE - 1) / GS_SLICE;
    if (np > 0x7fffffff) return MST_ERR_ARG;
    const int shift = (int)(((uintptr_t)grads & 15) / 4);
    const int vec = !grads2 || (((uintptr_t)grads2 & 15) == ((uintptr_t)grads & 15));
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)np), dim3(GS_THREADS), 0, s, grads, grads2, n, shift, vec, (double*)scratch);
    return np;
}

extern "C" int32_t mst_grad_norm(const float* grads, const float* grads2, int64_t n, void* scratch, float* norm, mst_stream stream) {
    if (!norm) return MST_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int64_t np = gs_launch_sumsq(grads, grads2, n, scratch, s);
    if (np < 0) return (int32_t)np;
    hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(GS_THREADS), 0, s, (const double*)scratch, np, norm);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

extern "C" int32_t mst_grad_norms(const float* grads, const float* grads2, const int64_t* offsets, const int64_t* lengths,
                                  int32_t count, float* norms, mst_stream stream) {
    if (!grads || !offsets || !lengths || !norms || count <= 0 || ((uintptr_t)grads & 3) || ((uintptr_t)grads2 & 3)) return MST_ERR_ARG;
    hipLaunchKernelGGL(grad_norms_kernel, dim3((unsigned)count), dim3(GS_THREADS), 0, (hipStream_t)stream, grads, grads2, offsets,
                       lengths, norms);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

extern "C" int32_t mst_adam_step_guarded(float* params, float* grads, float* grads2, float* exp_avg, float* exp_avg_sq, int64_t n,
                                         float* state, float* guard, void* scratch, double lr0, double beta1, double beta2,
                                         double eps, int32_t step_size, double gamma, double max_norm, int32_t skip_nonfinite,
                                         int32_t zero_grad, mst_stream stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !state || !guard || n <= 0 || step_size <= 0 || max_norm != max_norm)
        return MST_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int64_t np = gs_launch_sumsq(grads, grads2, n, scratch, s);
    if (np < 0) return (int32_t)np;
    const int clip = max_norm > 0.0 && max_norm <= 3.4028234663852886e38;      // <= 0, +inf or beyond fp32: no clipping
    hipLaunchKernelGGL(adam_prepare_guarded_kernel, dim3(1), dim3(GS_THREADS), 0, s, state, guard, (const double*)scratch, np, lr0,
                       beta1, beta2, (int)step_size, gamma, clip ? (float)max_norm : 0.f, clip, (int)(skip_nonfinite != 0));
    int64_t nb = (n + 1023) / 1024;
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(adam_guarded_kernel, dim3((unsigned)nb), dim3(256), 0, s, params, grads, grads2, exp_avg, exp_avg_sq, n,
                       (const float*)state, (const float*)guard, (float)beta1, (float)beta2, (float)eps, (int)zero_grad);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

// ------------------------------------------------------------------ hard_output
__global__ __launch_bounds__(256) void hard_output_kernel(float* x, float* out, int64_t n, int nf) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float* xi = x + i * nf;
        float* o = out + i * nf;
        o[0] = xi[0];
        const float vel = xi[1] > .01f ? xi[1] : 0.f;   // velocity *= (velocity > .01), in place on the input too
        xi[1] = vel;
        o[1] = vel;
        if (nf > 2) {
            const float mx = fmaxf(xi[2], fmaxf(xi[3], xi[4]));
            for (int a = 2; a < 5; ++a) o[a] = (xi[a] == mx && xi[a] > .1f) ? 1.f : 0.f;
        }
    }
}

extern "C" int32_t mst_hard_output(float* x, float* out, int64_t n_pos, int32_t nfeat, mst_stream stream) {
    if (!x || !out || n_pos <= 0 || (nfeat != 5 && nfeat != 2)) return MST_ERR_ARG;
    int64_t nb = (n_pos + 1023) / 1024;
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(hard_output_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, out, n_pos, (int)nfeat);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

// ------------------------------------------------------------------ sparse clip input (mst_clip_scatter)
// A clip arrives as sorted (cell, features) records; the dense note tensor the kernels read is built here.  The destination is cut
// into 16-byte-aligned slices of SCAT_SLICE floats, one workgroup each: the workgroup zero-fills an LDS image of its slice, drops the
// records that fall into the slice into the image and streams the image out with 16-byte stores.  Every float of the destination is
// written exactly once, by the one workgroup that owns it: no atomics, no clearing pass, stale or NaN contents never read.
#define SCAT_SLICE 2048          // floats per workgroup: 8 KB of LDS, two 16-byte stores per lane
#define SCAT_THREADS 256

// Lower bounds of two targets in the ascending cells[0, n), found by the whole workgroup: per round every lane samples the last cell
// of its 1/256 share of the remaining range, so two dependent loads settle up to 64 k records (a per-lane binary search is a chain
// of ~13).  Both searches share the barriers.  On cells that are not ascending the result is some index in [0, n]: the caller
// bounds-checks every record it stores.
__device__ __forceinline__ void scatter_bounds(const int32_t* cells, int n, int t0, int t1, int* flag, int* sel, int& lb0, int& lb1) {
    const int tid = threadIdx.x;
    int64_t a[2] = {0, 0}, b[2] = {n, n};
    const int tg[2] = {t0, t1};
    while (b[0] > a[0] || b[1] > a[1]) {           // workgroup-uniform
        int64_t s[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int64_t len = b[j] - a[j];
            s[j] = (len + SCAT_THREADS - 1) / SCAT_THREADS;
            const int64_t idx = a[j] + (int64_t)tid * s[j] + s[j] - 1;
            flag[j * SCAT_THREADS + tid] = (len > 0 && idx < b[j] && cells[idx] < tg[j]) ? 1 : 0;
        }
        if (tid < 2) sel[tid] = 0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j)                // the last lane whose sample is still below the target
            if (flag[j * SCAT_THREADS + tid] && (tid == SCAT_THREADS - 1 || !flag[j * SCAT_THREADS + tid + 1])) sel[j] = tid + 1;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (b[j] > a[j]) {
                const int64_t na = a[j] + (int64_t)sel[j] * s[j], nb = na + s[j] - 1;
                a[j] = na < b[j] ? na : b[j];
                b[j] = nb < b[j] ? nb : b[j];
            }
        }
        __syncthreads();                           // flag / sel are rewritten by the next round
    }
    lb0 = (int)a[0];
    lb1 = (int)a[1];
}

// grid = slices of the shifted flat destination: g = flat index + shift, shift = floats between the previous 16-byte boundary and
// out, so that g = 0 (mod 4) is a 16-byte-aligned address whatever the alignment of out
template <int NFEAT>
__global__ __launch_bounds__(SCAT_THREADS) void clip_scatter_kernel(const int32_t* cells, const float* feats, const int32_t* counts,
                                                                    int capacity, int64_t n_cells, int64_t total, float* out, int shift) {
    __shared__ float4 img4[SCAT_SLICE / 4];
    __shared__ int flag[2 * SCAT_THREADS], sel[2];
    float* img = reinterpret_cast<float*>(img4);
    const int tid = threadIdx.x;
    const int64_t gb = (int64_t)blockIdx.x * SCAT_SLICE;
    const int64_t g0 = gb > shift ? gb : shift;
    const int64_t g1 = gb + SCAT_SLICE < shift + total ? gb + SCAT_SLICE : shift + total;
    for (int i = tid; i < SCAT_SLICE / 4; i += SCAT_THREADS) img4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    const int64_t per = n_cells * NFEAT, f0 = g0 - shift, f1 = g1 - shift;
    for (int64_t k = f0 / per; k * per < f1; ++k) {                  // the clips this slice touches (one, or two at a seam)
        const int64_t lo = f0 > k * per ? f0 - k * per : 0;          // clip-local floats [lo, hi) of this slice
        const int64_t hi = f1 - k * per < per ? f1 - k * per : per;
        int n = counts[k];
        n = n < 0 ? 0 : (n > capacity ? capacity : n);               // whatever lies beyond the count is ignored
        const int32_t* ck = cells + k * capacity;
        const float* fk = feats + k * (int64_t)capacity * NFEAT;
        int r0, r1;                                                   // records of the cells that overlap [lo, hi)
        scatter_bounds(ck, n, (int)(lo / NFEAT), (int)((hi + NFEAT - 1) / NFEAT), flag, sel, r0, r1);
        for (int64_t e = tid; e < (int64_t)(r1 - r0) * NFEAT; e += SCAT_THREADS) {
            const int64_t r = r0 + e / NFEAT;
            const int64_t local = (int64_t)ck[r] * NFEAT + e % NFEAT;
            // a cell that straddles the slice edge is shared float by float; a cell >= n_cells has local >= per >= hi
            if (local >= lo && local < hi) img[k * per + local + shift - gb] = fk[r * NFEAT + e % NFEAT];
        }
    }
    __syncthreads();
    for (int i = tid; i < SCAT_SLICE / 4; i += SCAT_THREADS) {
        const int64_t g = gb + 4 * i;
        if (g >= g0 && g + 4 <= g1) {
            *reinterpret_cast<float4*>(out + (g - shift)) = img4[i];
        } else {                                                      // the ragged head and tail of the destination
            for (int j = 0; j < 4; ++j)
                if (g + j >= g0 && g + j < g1) out[g + j - shift] = img[4 * i + j];
        }
    }
}

extern "C" int32_t mst_clip_scatter(const int32_t* cells, const float* feats, const int32_t* counts, int32_t capacity,
                                    int32_t n_clips, int64_t n_cells, int32_t nfeat, float* out, mst_stream stream) {
    if (!cells || !feats || !counts || !out || capacity < 0 || n_clips < 1 || n_cells < 1 || n_cells >= ((int64_t)1 << 31) ||
        (nfeat != 5 && nfeat != 2) || ((uintptr_t)out & 3))
        return MST_ERR_ARG;
    const int shift = (int)(((uintptr_t)out & 15) / 4);
    const int64_t total = (int64_t)n_clips * n_cells * nfeat;
    const int64_t nb = (shift + total + SCAT_SLICE - 1) / SCAT_SLICE;
    if (nb > 0x7fffffff) return MST_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (nfeat == 5)
        hipLaunchKernelGGL(clip_scatter_kernel<5>, dim3((unsigned)nb), dim3(SCAT_THREADS), 0, s, cells, feats, counts, (int)capacity,
                           n_cells, total, out, shift);
    else
        hipLaunchKernelGGL(clip_scatter_kernel<2>, dim3((unsigned)nb), dim3(SCAT_THREADS), 0, s, cells, feats, counts, (int)capacity,
                           n_cells, total, out, shift);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

// ------------------------------------------------------------------ windowed clips (mst_clip_window)
// K clips of one shape cropped out of songs of any length whose records sit in a device pool.  The destination is cut into the
// same slices as above.  A (clip, channel) SLAB of it — bars x bar_cells cells — is the source cells [t0, t1) of that song's
// channel shifted by a constant, so a slice runs one search pair per slab it overlaps (several at the smallest shapes: an
// unpitched slab of one bar at T = 1 is 940 floats) and drops the records found into its LDS image exactly as the scatter does.
// The descriptors are read here, on the device: a captured launch replays with other songs and windows.
template <int NFEAT>
__global__ __launch_bounds__(SCAT_THREADS) void clip_window_kernel(const int32_t* cells, const float* feats, const mst_window* win,
                                                                   int channels, int bars, int64_t bar_cells, int64_t total,
                                                                   float* out, int shift) {
    __shared__ float4 img4[SCAT_SLICE / 4];
    __shared__ int flag[2 * SCAT_THREADS], sel[2];
    float* img = reinterpret_cast<float*>(img4);
    const int tid = threadIdx.x;
    const int64_t gb = (int64_t)blockIdx.x * SCAT_SLICE;
    const int64_t g0 = gb > shift ? gb : shift;
    const int64_t g1 = gb + SCAT_SLICE < shift + total ? gb + SCAT_SLICE : shift + total;
    for (int i = tid; i < SCAT_SLICE / 4; i += SCAT_THREADS) img4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    const int64_t slab_cells = (int64_t)bars * bar_cells, per = slab_cells * NFEAT, f0 = g0 - shift, f1 = g1 - shift;
    for (int64_t s = f0 / per; s * per < f1; ++s) {                  // the slabs this slice touches; everything here is uniform
        const int64_t lo = f0 > s * per ? f0 - s * per : 0;          // slab-local floats [lo, hi) of this slice
        const int64_t hi = f1 - s * per < per ? f1 - s * per : per;
        const mst_window w = win[s / channels];
        const int64_t c = s % channels;
        const int64_t roll_bars = (int64_t)channels * w.src_bars;    // a song of 2^31 cells or more has no int32 cell indices
        if (w.count <= 0 || w.first < 0 || w.src_bars < 1 || roll_bars >= ((int64_t)1 << 31) ||
            roll_bars * bar_cells >= ((int64_t)1 << 31))
            continue;
        // slab-local cells [d0, d1): those of the slice whose bar r0 + d / bar_cells exists in the song
        const int64_t v0 = w.r0 < 0 ? -(int64_t)w.r0 * bar_cells : 0;
        const int64_t left = (int64_t)w.src_bars - w.r0;             // bars of the song from r0 on (<= 0: wholly past the end)
        const int64_t v1 = left <= 0 ? 0 : (left < bars ? left * bar_cells : slab_cells);
        int64_t d0 = lo / NFEAT, d1 = (hi + NFEAT - 1) / NFEAT;
        d0 = d0 > v0 ? d0 : v0;
        d1 = d1 < v1 ? d1 : v1;
        if (d0 >= d1) continue;
        const int64_t off = (c * w.src_bars + w.r0) * bar_cells;     // source cell = slab-local cell + off, in [0, roll_cells)
        const int t0 = (int)(d0 + off), t1 = (int)(d1 + off);
        const int32_t* ck = cells + w.first;
        const float* fk = feats + (int64_t)w.first * NFEAT;
        int r0, r1;
        scatter_bounds(ck, w.count, t0, t1, flag, sel, r0, r1);
        for (int64_t e = tid; e < (int64_t)(r1 - r0) * NFEAT; e += SCAT_THREADS) {
            const int64_t r = r0 + e / NFEAT;
            const int64_t cell = ck[r];
            const int64_t local = (cell - off) * NFEAT + e % NFEAT;
            // on cells that are not ascending the search may hand over anything: only a cell of [t0, t1) is a cell of this slab
            if (cell >= t0 && cell < t1 && local >= lo && local < hi) img[s * per + local + shift - gb] = fk[r * NFEAT + e % NFEAT];
        }
    }
    __syncthreads();
    for (int i = tid; i < SCAT_SLICE / 4; i += SCAT_THREADS) {
        const int64_t g = gb + 4 * i;
        if (g >= g0 && g + 4 <= g1) {
            *reinterpret_cast<float4*>(out + (g - shift)) = img4[i];
        } else {                                                      // the ragged head and tail of the destination
            for (int j = 0; j < 4; ++j)
                if (g + j >= g0 && g + j < g1) out[g + j - shift] = img[4 * i + j];
        }
    }
}

extern "C" int32_t mst_clip_window(const int32_t* cells, const float* feats, const mst_window* win, int32_t n_clips, int32_t channels,
                                   int32_t bars, int64_t bar_cells, int32_t nfeat, float* out, mst_stream stream) {
    if (!cells || !feats || !win || !out || n_clips < 1 || channels < 1 || bars < 1 || bar_cells < 1 || (nfeat != 5 && nfeat != 2) ||
        ((uintptr_t)out & 3))
        return MST_ERR_ARG;
    if (bar_cells >= ((int64_t)1 << 31) || (int64_t)channels * bars >= ((int64_t)1 << 31) ||
        (int64_t)channels * bars * bar_cells >= ((int64_t)1 << 31))
        return MST_ERR_ARG;
    const int shift = (int)(((uintptr_t)out & 15) / 4);
    const int64_t total = (int64_t)n_clips * channels * bars * bar_cells * nfeat;
    const int64_t nb = (shift + total + SCAT_SLICE - 1) / SCAT_SLICE;
    if (nb > 0x7fffffff) return MST_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (nfeat == 5)
        hipLaunchKernelGGL(clip_window_kernel<5>, dim3((unsigned)nb), dim3(SCAT_THREADS), 0, s, cells, feats, win, (int)channels,
                           (int)bars, bar_cells, total, out, shift);
    else
        hipLaunchKernelGGL(clip_window_kernel<2>, dim3((unsigned)nb), dim3(SCAT_THREADS), 0, s, cells, feats, win, (int)channels,
                           (int)bars, bar_cells, total, out, shift);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

// ------------------------------------------------------------------ rotating song store (mst_store_admit)
// One refresh of a SongStore ring: a staged blob — a header of segments, then their payload — is copied into the store's pools
// and tables, bit for bit, in ONE launch whose arguments never change.  The header is read here, on the device, ADMIT_BATCH
// segments at a time: every lane checks one segment and counts its chunks of ADMIT_CHUNK words, the workgroup scans the counts
// in LDS, and the fixed grid strides over the batch's chunks (a table row is one chunk, a feats array a hundred).  A chunk is cut
// on the DESTINATION's 16-byte grid (`shift`, as the scatter cuts its slices): where source and destination are 16 bytes apart
// modulo 16 a lane moves four words with one 16-byte load and store, the ragged head and tail word by word; where they are not,
// the chunk goes word by word, a wave reading and writing consecutive words.  Words travel as integers: NaN payloads and -0.0
// arrive as they left.  Workgroup 0 writes the status words, every one of them on every launch.
#define ADMIT_THREADS 256
#define ADMIT_BATCH 256          // segments checked per round: one per lane
#define ADMIT_CHUNK 1024         // words per chunk: one 16-byte move per lane

struct alignas(16) admit_word4 { int32_t x, y, z, w; };
struct admit_dsts { int32_t* ptr[MST_ADMIT_DSTS]; int64_t words[MST_ADMIT_DSTS]; };

__global__ __launch_bounds__(ADMIT_THREADS) void store_admit_kernel(const int32_t* blob, int64_t blob_words, int max_segments,
                                                                    admit_dsts dsts, int32_t* status) {
    __shared__ int s_scan[2][ADMIT_BATCH];                 // inclusive prefix of the batch's chunk counts (double-buffered scan)
    __shared__ int s_dst[ADMIT_BATCH], s_dst_off[ADMIT_BATCH], s_src_off[ADMIT_BATCH], s_words[ADMIT_BATCH];
    const int tid = threadIdx.x;
    int n = blob[0];
    n = n < 0 ? 0 : (n > max_segments ? max_segments : n);
    const int64_t payload = 4 + 4 * (int64_t)max_segments;
    for (int base = 0; base < max_segments; base += ADMIT_BATCH) {      // workgroup-uniform
        const int i = base + tid;
        int chunks = 0;
        mst_segment sg = {0, 0, 0, 0};
        if (i < max_segments) {
            int refused = 0;
            if (i < n) {
                sg = *reinterpret_cast<const mst_segment*>(blob + 4 + 4 * (int64_t)i);
                const int64_t w = sg.words;
                bool ok = sg.dst >= 0 && sg.dst < MST_ADMIT_DSTS && w >= 0 && sg.src_off >= payload && sg.src_off + w <= blob_words &&
                          sg.dst_off >= 0;
                if (ok) ok = dsts.ptr[sg.dst] != nullptr && sg.dst_off + w <= dsts.words[sg.dst];
                refused = ok ? 0 : 1;
                if (ok && w > 0) {
                    const int shift = (int)(((uintptr_t)(dsts.ptr[sg.dst] + sg.dst_off) & 15) / 4);
                    chunks = (int)((shift + w + ADMIT_CHUNK - 1) / ADMIT_CHUNK);
                }
            }
            if (blockIdx.x == 0) status[i] = refused;
        }
        s_dst[tid] = sg.dst;
        s_dst_off[tid] = sg.dst_off;
        s_src_off[tid] = sg.src_off;
        s_words[tid] = sg.words;                           // read only where the segment has chunks, i.e. was accepted
        s_scan[0][tid] = chunks;
        __syncthreads();
        int cur = 0;
        for (int d = 1; d < ADMIT_BATCH; d <<= 1) {        // Hillis-Steele: a batch of 256 chunk counts sums below 2^31
            s_scan[cur ^ 1][tid] = s_scan[cur][tid] + (tid >= d ? s_scan[cur][tid - d] : 0);
            cur ^= 1;
            __syncthreads();
        }
        const int* pre = s_scan[cur];
        const int total = pre[ADMIT_BATCH - 1];
        for (int g = blockIdx.x; g < total; g += gridDim.x) {           // workgroup-uniform
            int lo = 0, hi = ADMIT_BATCH - 1;              // the first segment whose inclusive prefix exceeds g
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (pre[mid] > g) hi = mid; else lo = mid + 1;
            }
            const int c = g - (lo ? pre[lo - 1] : 0);
            const int32_t* src = blob + s_src_off[lo];
            int32_t* dst = dsts.ptr[s_dst[lo]] + s_dst_off[lo];
            const int64_t words = s_words[lo];
            const int shift = (int)(((uintptr_t)dst & 15) / 4);
            // v = word index + shift: v = 0 (mod 4) is a 16-byte boundary of the destination
            const int64_t v0 = (int64_t)c * ADMIT_CHUNK, vend = shift + words;
            if ((((uintptr_t)src ^ (uintptr_t)dst) & 15) == 0) {
                const int64_t v = v0 + 4 * tid;
                if (v >= shift && v + 4 <= vend) {
                    *reinterpret_cast<admit_word4*>(dst + (v - shift)) = *reinterpret_cast<const admit_word4*>(src + (v - shift));
                } else {                                                // the ragged head and tail of the segment
                    for (int j = 0; j < 4; ++j)
                        if (v + j >= shift && v + j < vend) dst[v + j - shift] = src[v + j - shift];
                }
            } else {
                for (int j = 0; j < ADMIT_CHUNK / ADMIT_THREADS; ++j) {
                    const int64_t v = v0 + j * ADMIT_THREADS + tid;
                    if (v >= shift && v < vend) dst[v - shift] = src[v - shift];
                }
            }
        }
        __syncthreads();                                   // the LDS tables are rewritten by the next batch
    }
}

// compute units of the current device, asked once per device (the grid of mst_store_admit is sized from it)
static int admit_cus() {
#ifdef HIPSIM
    return 4;
#else
    static int cached[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 0;
    if (dev < 64 && cached[dev] > 0) return cached[dev];
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    if (dev < 64) cached[dev] = cus;
    return cus;
#endif
}

extern "C" int32_t mst_store_admit(const int32_t* blob, int64_t blob_words, int32_t max_segments, void* const dst[MST_ADMIT_DSTS],
                                   const int64_t dst_words[MST_ADMIT_DSTS], int32_t* status, mst_stream stream) {
    if (!blob || !dst || !dst_words || !status || max_segments < 1 || blob_words < 4 + 4 * (int64_t)max_segments ||
        ((uintptr_t)blob & 3) || ((uintptr_t)status & 3))
        return MST_ERR_ARG;
    admit_dsts d;
    for (int k = 0; k < MST_ADMIT_DSTS; ++k) {
        if ((uintptr_t)dst[k] & 3) return MST_ERR_ARG;
        d.ptr[k] = static_cast<int32_t*>(dst[k]);
        d.words[k] = dst_words[k];
    }
    const int cus = admit_cus();
    if (cus < 1) return MST_ERR_LAUNCH;
    // two workgroups per compute unit: a refresh of a few songs is some hundred chunks, and 512 lanes keep a CU's loads in flight
    hipLaunchKernelGGL(store_admit_kernel, dim3((unsigned)(2 * cus)), dim3(ADMIT_THREADS), 0, (hipStream_t)stream, blob, blob_words,
                       (int)max_segments, d, status);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

// ------------------------------------------------------------------ sparse clip output (mst_roll_count, mst_roll_compact)
// The inverse of the scatter: the sorted (cell, features) records of a dense roll, so that only the notes go back to the host.
// An ordered stream compaction in the usual three steps — per-slice counts, an exclusive scan of the counts, emit — with no atomics
// and no workgroup waiting for another: the records, and their order, are the same bits on every run.  One workgroup owns a slice
// of ROLL_SLICE consecutive cells.  A cell is 20 or 8 bytes, so a lane loading "its" cell would issue unaligned strided loads:
// the workgroup stages the slice into LDS with 16-byte loads instead and evaluates the predicate from the image.  The emit pass
// reads the slice a second time and recomputes the predicate (no per-cell mask is kept), packs the records in LDS in cell order
// and streams them out contiguously.
#define ROLL_SLICE 1024          // cells per workgroup: 20 KB of LDS at five features
#define ROLL_THREADS 256
#define ROLL_WAVES (ROLL_THREADS / 64)
#define ROLL_PER_LANE (ROLL_SLICE / ROLL_THREADS)
typedef float roll_f4 __attribute__((ext_vector_type(4)));

extern "C" int64_t mst_roll_slices(int64_t n_cells) {
    if (n_cells < 1 || n_cells >= ((int64_t)1 << 31)) return MST_ERR_ARG;
    return (n_cells + ROLL_SLICE - 1) / ROLL_SLICE;
}

// Stages slice `slice` into LDS and returns its number of cells (the last slice is ragged).  g = flat float index + shift,
// shift = floats between the previous 16-byte boundary and x, so that g = 0 (mod 4) is a 16-byte-aligned address whatever the
// alignment of x.  img4 holds g in [gb, gb + ROLL_SLICE * NFEAT + 4); cell c of the slice starts at float shift + c * NFEAT of it.
// Only floats of x are read: a group of four that is not wholly inside the slice takes scalar loads.
template <int NFEAT>
__device__ __forceinline__ int roll_stage(const float* x, int64_t n_cells, int shift, roll_f4* img4, int slice = blockIdx.x) {
    float* img = reinterpret_cast<float*>(img4);
    const MST_GLOBAL_AS float* xg = (const MST_GLOBAL_AS float*)x;
    const int64_t c0 = (int64_t)slice * ROLL_SLICE;
    const int cells = (int)(n_cells - c0 < ROLL_SLICE ? n_cells - c0 : ROLL_SLICE);
    const int64_t gb = c0 * NFEAT, g0 = gb + shift, g1 = g0 + (int64_t)cells * NFEAT;
    for (int i = threadIdx.x; i < ROLL_SLICE * NFEAT / 4 + 1; i += ROLL_THREADS) {
        const int64_t g = gb + 4 * i;
        if (g >= g0 && g + 4 <= g1) {
            img4[i] = *reinterpret_cast<const MST_GLOBAL_AS roll_f4*>(xg + (g - shift));
        } else {
            for (int j = 0; j < 4; ++j)
                if (g + j >= g0 && g + j < g1) img[4 * i + j] = xg[g + j - shift];
        }
    }
    __syncthreads();
    return cells;
}

// Is cell `c` a record, and with which features?  MST_ROLL_NONZERO: any non-zero bit pattern (-0.0 and NaN count), features
// verbatim.  MST_ROLL_HARD: hard_output_kernel's operations in its order (style/model.py:818-832); a record when the hard
// velocity is non-zero, so a NaN velocity is dropped as hard_output zeroes it.
template <int NFEAT>
__device__ __forceinline__ bool roll_record(const float* c, int mode, float (&f)[NFEAT]) {
    if (mode == MST_ROLL_NONZERO) {
        unsigned any = 0;
#pragma unroll
        for (int k = 0; k < NFEAT; ++k) {
            f[k] = c[k];
            any |= __float_as_uint(c[k]);
        }
        return any != 0;
    }
    f[0] = c[0];
    f[1] = c[1] > .01f ? c[1] : 0.f;
    if (NFEAT > 2) {
        const float mx = fmaxf(c[2], fmaxf(c[3], c[4]));
#pragma unroll
        for (int a = 2; a < NFEAT; ++a) f[a] = (c[a] == mx && c[a] > .1f) ? 1.f : 0.f;
    }
    return c[1] > .01f;
}

// inclusive scan over the 64 lanes of a wave
__device__ __forceinline__ int roll_wave_scan(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl(v, lane >= d ? lane - d : lane);
        if (lane >= d) v += t;
    }
    return v;
}

// Wave w owns cells [256 w, 256 w + 256) of the slice and lane l the cells 256 w + 64 j + l, j < 4: neighbouring lanes read
// neighbouring cells, 5 (or 2) floats apart in LDS — an odd stride is conflict-free for ds_read_b32, the unpitched stride of 2
// costs two LDS cycles per read.
#define ROLL_CELL(wave, j, lane) ((wave) * (64 * ROLL_PER_LANE) + (j) * 64 + (lane))

// the records of slice `slice` of the roll at x, counted into ws[slice]: the body of the one-roll and of the batched kernel
template <int NFEAT>
__device__ __forceinline__ void roll_count_slice(const float* x, int64_t n_cells, int shift, int mode, int slice, int32_t* ws) {
    __shared__ roll_f4 img4[ROLL_SLICE * NFEAT / 4 + 1];
    __shared__ int wtot[ROLL_WAVES];
    const int cells = roll_stage<NFEAT>(x, n_cells, shift, img4, slice);
    const float* img = reinterpret_cast<const float*>(img4) + shift;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int n = 0;
#pragma unroll
    for (int j = 0; j < ROLL_PER_LANE; ++j) {
        const int c = ROLL_CELL(wave, j, lane);
        float f[NFEAT];
        if (c < cells && roll_record<NFEAT>(img + c * NFEAT, mode, f)) ++n;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if (lane == 0) wtot[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < ROLL_WAVES; ++w) total += wtot[w];
        ws[slice] = total;
    }
}

template <int NFEAT>
__global__ __launch_bounds__(ROLL_THREADS) void roll_count_kernel(const float* x, int64_t n_cells, int shift, int mode, int32_t* ws) {
    roll_count_slice<NFEAT>(x, n_cells, shift, mode, blockIdx.x, ws);
}

// The batched twin: workgroup (s, y) owns slice s of roll r0 + y, the n_cells x NFEAT floats at x + (r0 + y) * roll_stride, and
// row r0 + y of ws (slices + 1 words).  The roll's 16-byte phase is its own: roll_stride need not be a multiple of 4.
template <int NFEAT>
__global__ __launch_bounds__(ROLL_THREADS) void rolls_count_kernel(const float* x, int64_t roll_stride, int64_t r0, int64_t n_cells, int mode,
                                                                   int32_t* ws) {
    const int64_t k = r0 + blockIdx.y;
    const float* xk = x + k * roll_stride;
    roll_count_slice<NFEAT>(xk, n_cells, (int)(((uintptr_t)xk & 15) / 4), mode, blockIdx.x, ws + k * ((int64_t)gridDim.x + 1));
}

// one workgroup: ws[0, n) from per-slice counts to their exclusive prefix, in place and in order; ws[n] = the total
__device__ __forceinline__ void roll_scan_row(int32_t* ws, int n) {
    __shared__ int wtot[ROLL_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int carry = 0;
    for (int base = 0; base < n; base += ROLL_THREADS * 4) {       // workgroup-uniform
        const int i0 = base + tid * 4;
        int v[4], sum = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = i0 + j < n ? ws[i0 + j] : 0;
            sum += v[j];
        }
        const int incl = roll_wave_scan(sum, lane);
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        int run = carry + incl - sum, total = 0;
        for (int w = 0; w < ROLL_WAVES; ++w) {
            if (w < wave) run += wtot[w];
            total += wtot[w];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i0 + j < n) ws[i0 + j] = run;
            run += v[j];
        }
        carry += total;
        __syncthreads();                                           // wtot is rewritten by the next round
    }
    if (tid == 0) ws[n] = carry;
}

__global__ __launch_bounds__(ROLL_THREADS) void roll_scan_kernel(int32_t* ws, int n) { roll_scan_row(ws, n); }

// the batched twin: workgroup k scans row k of ws (n + 1 words)
__global__ __launch_bounds__(ROLL_THREADS) void rolls_scan_kernel(int32_t* ws, int n) {
    roll_scan_row(ws + (int64_t)blockIdx.x * ((int64_t)n + 1), n);
}

// the records of slice `slice` of the roll at x, written behind those of the slices before it: the body of both emit kernels
template <int NFEAT>
__device__ __forceinline__ void roll_emit_slice(const float* x, int64_t n_cells, int shift, int mode, int slice, const int32_t* ws,
                                                int64_t capacity, int32_t* cells_out, float* feats) {
    __shared__ roll_f4 img4[ROLL_SLICE * NFEAT / 4 + 1];
    __shared__ int32_t rec[ROLL_SLICE];
    __shared__ int wtot[ROLL_WAVES];
    const int base = ws[slice];                                    // records in the slices before this one
    if (base < 0 || base >= capacity || ws[slice + 1] == base) return;          // nothing of this slice is stored (workgroup-uniform)
    const int cells = roll_stage<NFEAT>(x, n_cells, shift, img4, slice);
    float* img = reinterpret_cast<float*>(img4);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // one byte per j: is the lane's j-th cell a record?  Scanned over the wave as one integer (a byte counts to 64 at most).
    float f[ROLL_PER_LANE][NFEAT];
    int mine = 0;
#pragma unroll
    for (int j = 0; j < ROLL_PER_LANE; ++j) {
        const int c = ROLL_CELL(wave, j, lane);
        if (c < cells && roll_record<NFEAT>(img + shift + c * NFEAT, mode, f[j])) mine |= 1 << (8 * j);
    }
    const int incl = roll_wave_scan(mine, lane);
    const int tot = __shfl(incl, 63);
    if (lane == 0) wtot[wave] = (tot & 255) + ((tot >> 8) & 255) + ((tot >> 16) & 255) + ((tot >> 24) & 255);
    __syncthreads();                                               // and every lane holds its cells in registers: the image may be overwritten
    int rank = 0, count = 0;
    for (int w = 0; w < ROLL_WAVES; ++w) {
        if (w < wave) rank += wtot[w];
        count += wtot[w];
    }
    const int32_t c0 = (int32_t)((int64_t)slice * ROLL_SLICE);
#pragma unroll
    for (int j = 0; j < ROLL_PER_LANE; ++j) {                      // cell order within the wave: j, then lane
        if ((mine >> (8 * j)) & 1) {
            const int r = rank + ((incl >> (8 * j)) & 255) - 1;
            rec[r] = c0 + ROLL_CELL(wave, j, lane);
#pragma unroll
            for (int k = 0; k < NFEAT; ++k) img[r * NFEAT + k] = f[j][k];
        }
        rank += (tot >> (8 * j)) & 255;
    }
    __syncthreads();
    const int64_t room = capacity - base;                          // records of rank >= capacity are dropped, never stored
    const int keep = count < room ? count : (int)room;
    for (int i = tid; i < keep; i += ROLL_THREADS) cells_out[base + i] = rec[i];
    float* dst = feats + (int64_t)base * NFEAT;
    for (int i = tid; i < keep * NFEAT; i += ROLL_THREADS) dst[i] = img[i];
}

template <int NFEAT>
__global__ __launch_bounds__(ROLL_THREADS) void roll_emit_kernel(const float* x, int64_t n_cells, int shift, int mode, const int32_t* ws,
                                                                 int64_t capacity, int32_t* cells_out, float* feats) {
    roll_emit_slice<NFEAT>(x, n_cells, shift, mode, blockIdx.x, ws, capacity, cells_out, feats);
}

// The batched twin: workgroup (s, y) emits slice s of roll k = r0 + y into row k of cells / feats (capacity records each).  The
// first workgroup of a roll also leaves the roll's TRUE total in counts[k], before anything can make it return.
template <int NFEAT>
__global__ __launch_bounds__(ROLL_THREADS) void rolls_emit_kernel(const float* x, int64_t roll_stride, int64_t r0, int64_t n_cells, int mode,
                                                                  const int32_t* ws, int capacity, int32_t* cells_out, float* feats,
                                                                  int32_t* counts) {
    const int64_t k = r0 + blockIdx.y;
    const float* xk = x + k * roll_stride;
    const int32_t* wsk = ws + k * ((int64_t)gridDim.x + 1);
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[k] = wsk[gridDim.x];
    roll_emit_slice<NFEAT>(xk, n_cells, (int)(((uintptr_t)xk & 15) / 4), mode, blockIdx.x, wsk, capacity, cells_out + k * capacity,
                           feats + k * capacity * NFEAT);
}

static bool roll_args_ok(const float* x, int64_t n_cells, int32_t nfeat, int32_t mode) {
    return x && n_cells >= 1 && n_cells < ((int64_t)1 << 31) && (nfeat == 5 || nfeat == 2) &&
           (mode == MST_ROLL_NONZERO || mode == MST_ROLL_HARD) && !((uintptr_t)x & 3);
}

extern "C" int32_t mst_roll_count(const float* x, int64_t n_cells, int32_t nfeat, int32_t mode, int32_t* ws, mst_stream stream) {
    if (!roll_args_ok(x, n_cells, nfeat, mode) || !ws) return MST_ERR_ARG;
    const int shift = (int)(((uintptr_t)x & 15) / 4);
    const unsigned nb = (unsigned)mst_roll_slices(n_cells);
    hipStream_t s = (hipStream_t)stream;
    if (nfeat == 5)
        hipLaunchKernelGGL(roll_count_kernel<5>, dim3(nb), dim3(ROLL_THREADS), 0, s, x, n_cells, shift, (int)mode, ws);
    else
        hipLaunchKernelGGL(roll_count_kernel<2>, dim3(nb), dim3(ROLL_THREADS), 0, s, x, n_cells, shift, (int)mode, ws);
    hipLaunchKernelGGL(roll_scan_kernel, dim3(1), dim3(ROLL_THREADS), 0, s, ws, (int)nb);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

extern "C" int32_t mst_roll_compact(const float* x, int64_t n_cells, int32_t nfeat, int32_t mode, const int32_t* ws, int64_t capacity,
                                    int32_t* cells, float* feats, mst_stream stream) {
    if (!roll_args_ok(x, n_cells, nfeat, mode) || !ws || !cells || !feats || capacity < 0) return MST_ERR_ARG;
    if (capacity == 0) return MST_OK;
    const int shift = (int)(((uintptr_t)x & 15) / 4);
    const unsigned nb = (unsigned)mst_roll_slices(n_cells);
    hipStream_t s = (hipStream_t)stream;
    if (nfeat == 5)
        hipLaunchKernelGGL(roll_emit_kernel<5>, dim3(nb), dim3(ROLL_THREADS), 0, s, x, n_cells, shift, (int)mode, ws, capacity, cells, feats);
    else
        hipLaunchKernelGGL(roll_emit_kernel<2>, dim3(nb), dim3(ROLL_THREADS), 0, s, x, n_cells, shift, (int)mode, ws, capacity, cells, feats);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

// ---- the batched, strided twins (mst_rolls_count, mst_rolls_compact): the K prediction rolls of a batched plan lie clip_stride
// floats apart in its workspace; one grid takes them all, the roll in blockIdx.y.
#define ROLLS_MAX_GRID_Y 65535   // rolls one launch takes in blockIdx.y; more rolls are more launches of the same chain

static bool rolls_args_ok(const float* x, int64_t roll_stride, int32_t n_rolls, int64_t n_cells, int32_t nfeat, int32_t mode) {
    return roll_args_ok(x, n_cells, nfeat, mode) && n_rolls >= 1 && roll_stride >= n_cells * nfeat &&
           (int64_t)n_rolls * mst_roll_slices(n_cells) < ((int64_t)1 << 31);
}

extern "C" int32_t mst_rolls_count(const float* x, int64_t roll_stride, int32_t n_rolls, int64_t n_cells, int32_t nfeat, int32_t mode,
                                   int32_t* ws, mst_stream stream) {
    if (!rolls_args_ok(x, roll_stride, n_rolls, n_cells, nfeat, mode) || !ws) return MST_ERR_ARG;
    const unsigned nb = (unsigned)mst_roll_slices(n_cells);
    hipStream_t s = (hipStream_t)stream;
    for (int64_t r0 = 0; r0 < n_rolls; r0 += ROLLS_MAX_GRID_Y) {
        const unsigned ny = (unsigned)(n_rolls - r0 < ROLLS_MAX_GRID_Y ? n_rolls - r0 : ROLLS_MAX_GRID_Y);
        if (nfeat == 5)
            hipLaunchKernelGGL(rolls_count_kernel<5>, dim3(nb, ny), dim3(ROLL_THREADS), 0, s, x, roll_stride, r0, n_cells, (int)mode, ws);
        else
            hipLaunchKernelGGL(rolls_count_kernel<2>, dim3(nb, ny), dim3(ROLL_THREADS), 0, s, x, roll_stride, r0, n_cells, (int)mode, ws);
    }
    hipLaunchKernelGGL(rolls_scan_kernel, dim3((unsigned)n_rolls), dim3(ROLL_THREADS), 0, s, ws, (int)nb);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

extern "C" int32_t mst_rolls_compact(const float* x, int64_t roll_stride, int32_t n_rolls, int64_t n_cells, int32_t nfeat, int32_t mode,
                                     const int32_t* ws, int32_t capacity, int32_t* cells, float* feats, int32_t* counts,
                                     mst_stream stream) {
    if (!rolls_args_ok(x, roll_stride, n_rolls, n_cells, nfeat, mode) || !ws || !cells || !feats || !counts || capacity < 0)
        return MST_ERR_ARG;
    const unsigned nb = (unsigned)mst_roll_slices(n_cells);
    hipStream_t s = (hipStream_t)stream;
    for (int64_t r0 = 0; r0 < n_rolls; r0 += ROLLS_MAX_GRID_Y) {
        const unsigned ny = (unsigned)(n_rolls - r0 < ROLLS_MAX_GRID_Y ? n_rolls - r0 : ROLLS_MAX_GRID_Y);
        if (nfeat == 5)
            hipLaunchKernelGGL(rolls_emit_kernel<5>, dim3(nb, ny), dim3(ROLL_THREADS), 0, s, x, roll_stride, r0, n_cells, (int)mode, ws,
                               (int)capacity, cells, feats, counts);
        else
            hipLaunchKernelGGL(rolls_emit_kernel<2>, dim3(nb, ny), dim3(ROLL_THREADS), 0, s, x, roll_stride, r0, n_cells, (int)mode, ws,
                               (int)capacity, cells, feats, counts);
    }
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

// ------------------------------------------------------------------ note metrics (mst_roll_metrics, mst_eval_iteration)
// How good are hard_output's decisions?  Prediction and target are streamed once, like roll_count_kernel streams one roll: a
// workgroup owns one slice of ROLL_SLICE cells of ONE group (a run of consecutive cells: a channel of a clip), stages the slice
// of both tensors into LDS with roll_stage (two images, 41 KB at five features; each tensor with the shift of its own group
// base, so the two may be misaligned differently and an odd group_cells only changes every second group's shift) and leaves one
// 32-byte partial: four counts and two double sums.  A second launch, one workgroup per group, adds the group's partials in a
// fixed order.  No atomics, no workgroup waits for another, the number of partials depends on the arguments alone: the same
// bits on every run.  The per-lane cell order is roll_count_kernel's (ROLL_CELL), the workgroup reduction grad_sumsq_kernel's.
struct MetricPartial { int32_t n_pred, n_tgt, tp, acc; double vel, dur; };
static_assert(sizeof(MetricPartial) == 32, "one 32-byte partial per slice");
#define METRIC_MAX_GRID_Y 65535  // groups one launch takes in blockIdx.y; more groups are more launches of the same chain

extern "C" int64_t mst_roll_metrics_scratch_bytes(int64_t n_groups, int64_t group_cells) {
    const int64_t slices = mst_roll_slices(group_cells);
    if (n_groups < 1 || slices < 1 || n_groups >= ((int64_t)1 << 31) || n_groups * slices >= ((int64_t)1 << 31)) return MST_ERR_ARG;
    return n_groups * slices * (int64_t)sizeof(MetricPartial);
}

// group g = g0 + blockIdx.y is channel g % gpc of clip g / gpc; a clip's groups are consecutive, clips sit pred_cs / tgt_cs
// floats apart (a plan's workspace slices against the caller's dense batch)
template <int NFEAT>
__global__ __launch_bounds__(ROLL_THREADS) void roll_metrics_kernel(const float* pred, const float* target, int64_t group_cells, int64_t g0,
                                                                    int gpc, int64_t pred_cs, int64_t tgt_cs, MetricPartial* partials) {
    __shared__ roll_f4 imgp4[ROLL_SLICE * NFEAT / 4 + 1];
    __shared__ roll_f4 imgt4[ROLL_SLICE * NFEAT / 4 + 1];
    __shared__ int redi[ROLL_WAVES][4];
    __shared__ double redd[ROLL_WAVES][2];
    const int64_t g = g0 + blockIdx.y;
    const float* pg = pred + (g / gpc) * pred_cs + (g % gpc) * group_cells * NFEAT;
    const float* tg = target + (g / gpc) * tgt_cs + (g % gpc) * group_cells * NFEAT;
    const int shp = (int)(((uintptr_t)pg & 15) / 4), sht = (int)(((uintptr_t)tg & 15) / 4);
    const int cells = roll_stage<NFEAT>(pg, group_cells, shp, imgp4);
    roll_stage<NFEAT>(tg, group_cells, sht, imgt4);
    const float* ip = reinterpret_cast<const float*>(imgp4) + shp;
    const float* it = reinterpret_cast<const float*>(imgt4) + sht;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int cnt[4] = {0, 0, 0, 0};
    double vel = 0.0, dur = 0.0;
#pragma unroll
    for (int j = 0; j < ROLL_PER_LANE; ++j) {
        const int c = ROLL_CELL(wave, j, lane);
        if (c >= cells) continue;
        const float* p = ip + c * NFEAT;
        const float* t = it + c * NFEAT;
        float hard[NFEAT];
        const bool on = roll_record<NFEAT>(p, MST_ROLL_HARD, hard);      // hard_output's decisions (a NaN velocity is off)
        const bool want = t[1] > 0.f;                                    // the loss's mask
        cnt[0] += on;
        cnt[1] += want;
        if (on && want) {
            ++cnt[2];
            if (NFEAT > 2) {
                bool same = true;
#pragma unroll
                for (int a = 2; a < NFEAT; ++a) same = same && hard[a] == t[a];
                cnt[3] += same;
            }
            vel += (double)fabsf(p[1] - t[1]);
            dur += (double)fabsf(p[0] - fminf(t[0], 6.f));               // get_duration_loss's clamp
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt[k] += __shfl_xor(cnt[k], o);
    }
    vel = wave_sum_d(vel);
    dur = wave_sum_d(dur);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) redi[wave][k] = cnt[k];
        redd[wave][0] = vel;
        redd[wave][1] = dur;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        MetricPartial m = {0, 0, 0, 0, 0.0, 0.0};
        for (int w = 0; w < ROLL_WAVES; ++w) {
            m.n_pred += redi[w][0]; m.n_tgt += redi[w][1]; m.tp += redi[w][2]; m.acc += redi[w][3];
            m.vel += redd[w][0]; m.dur += redd[w][1];
        }
        partials[g * gridDim.x + blockIdx.x] = m;
    }
}

// The whole workgroup: a group's partials in a fixed order (per-lane chains over q = lane, lane + 256, ..., a wave shuffle sum,
// the four wave sums in wave order) into one record.  Counts travel as doubles: integers below 2^53 are exact in any order.
__device__ __forceinline__ void metrics_finish_group(const MetricPartial* part, int64_t np, int64_t cells, double* rec) {
    __shared__ double red[6][ROLL_WAVES];
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t q = threadIdx.x; q < np; q += ROLL_THREADS) {
        const MetricPartial m = part[q];
        v[0] += (double)m.n_pred; v[1] += (double)m.n_tgt; v[2] += (double)m.tp; v[3] += (double)m.acc;
        v[4] += m.vel; v[5] += m.dur;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        v[k] = wave_sum_d(v[k]);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        rec[0] = (double)cells;
        for (int k = 0; k < 6; ++k) {
            double total = 0.0;
            for (int w = 0; w < ROLL_WAVES; ++w) total += red[k][w];
            rec[1 + k] = total;
        }
        rec[7] = 0.0;
    }
}

__global__ __launch_bounds__(ROLL_THREADS) void roll_metrics_finish_kernel(const MetricPartial* partials, int64_t slices, int64_t cells,
                                                                           double* out) {
    metrics_finish_group(partials + (int64_t)blockIdx.x * slices, slices, cells, out + (int64_t)blockIdx.x * MST_METRIC_WORDS);
}

// finishing launch of an evaluation iteration: workgroup b writes record b % (C + 2) of clip b / (C + 2) — a pitched channel,
// the unpitched roll (all zero without percussion) or the song-info record
__global__ __launch_bounds__(ROLL_THREADS) void eval_metrics_finish_kernel(EvalMetricsArgs a) {
    const int per = a.C + 2;
    const int64_t k = blockIdx.x / per;
    const int r = blockIdx.x % per;
    double* rec = a.out + (int64_t)blockIdx.x * MST_METRIC_WORDS;
    if (r < a.C) {
        metrics_finish_group((const MetricPartial*)a.part_p + (k * a.C + r) * a.slices_p, a.slices_p, a.cells_p, rec);
    } else if (r == a.C) {
        if (a.part_u) metrics_finish_group((const MetricPartial*)a.part_u + k * a.slices_u, a.slices_u, a.cells_u, rec);
        else if (threadIdx.x < MST_METRIC_WORDS) rec[threadIdx.x] = 0.0;
    } else if (threadIdx.x == 0) {
        const float* il = a.il + k * a.ws_stride; const float* it = a.it + k * a.ws_stride;
        const float* ml = a.mlg + k * a.ws_stride; const float* mt = a.mt + k * a.ws_stride;
        int n_pred = 0, n_tgt = 0, both = 0;
        for (int j = 0; j < a.ni; ++j) {
            const bool on = il[j] > 0.f, want = it[j] > .5f;
            n_pred += on; n_tgt += want; both += on && want;
        }
        rec[0] = (double)a.ni; rec[1] = (double)n_pred; rec[2] = (double)n_tgt; rec[3] = (double)both;
        rec[4] = (ml[1] > ml[0]) == (mt[1] > mt[0]) ? 1.0 : 0.0;       // first index of the largest of two
        rec[5] = (double)fabsf(a.bp[k * a.ws_stride] - a.bt[k * a.ws_stride]);
        rec[6] = rec[7] = 0.0;
    }
}

static bool roll_metrics_args_ok(const float* pred, const float* target, int64_t n_groups, int64_t group_cells, int32_t nfeat,
                                 const void* scratch) {
    return pred && target && scratch && (nfeat == 5 || nfeat == 2) && mst_roll_metrics_scratch_bytes(n_groups, group_cells) > 0 &&
           !((uintptr_t)pred & 3) && !((uintptr_t)target & 3) && !((uintptr_t)scratch & 7);
}

int launch_roll_metrics(const float* pred, const float* target, int64_t n_groups, int64_t group_cells, int nfeat, int gpc,
                        int64_t pred_cs, int64_t tgt_cs, void* scratch, hipStream_t s) {
    if (!roll_metrics_args_ok(pred, target, n_groups, group_cells, nfeat, scratch) || gpc < 1 || ((pred_cs | tgt_cs) < 0)) return MST_ERR_ARG;
    const unsigned nb = (unsigned)mst_roll_slices(group_cells);
    for (int64_t g0 = 0; g0 < n_groups; g0 += METRIC_MAX_GRID_Y) {
        const unsigned ny = (unsigned)(n_groups - g0 < METRIC_MAX_GRID_Y ? n_groups - g0 : METRIC_MAX_GRID_Y);
        if (nfeat == 5)
            hipLaunchKernelGGL(roll_metrics_kernel<5>, dim3(nb, ny), dim3(ROLL_THREADS), 0, s, pred, target, group_cells, g0, gpc, pred_cs,
                               tgt_cs, (MetricPartial*)scratch);
        else
            hipLaunchKernelGGL(roll_metrics_kernel<2>, dim3(nb, ny), dim3(ROLL_THREADS), 0, s, pred, target, group_cells, g0, gpc, pred_cs,
                               tgt_cs, (MetricPartial*)scratch);
    }
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

int launch_eval_metrics_finish(const EvalMetricsArgs& a, int clips, hipStream_t s) {
    hipLaunchKernelGGL(eval_metrics_finish_kernel, dim3((unsigned)(clips * (a.C + 2))), dim3(ROLL_THREADS), 0, s, a);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

extern "C" int32_t mst_roll_metrics(const float* pred, const float* target, int64_t n_groups, int64_t group_cells, int32_t nfeat,
                                    void* scratch, double* out, mst_stream stream) {
    if (!out || ((uintptr_t)out & 7)) return MST_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    // one clip of n_groups consecutive groups
    const int gpc = (int)(n_groups < 0x7fffffff ? n_groups : 0x7fffffff);
    const int e = launch_roll_metrics(pred, target, n_groups, group_cells, nfeat, gpc, 0, 0, scratch, s);
    if (e) return e;
    hipLaunchKernelGGL(roll_metrics_finish_kernel, dim3((unsigned)n_groups), dim3(ROLL_THREADS), 0, s, (const MetricPartial*)scratch,
                       mst_roll_slices(group_cells), group_cells, out);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

// ------------------------------------------------------------------ windowed evaluation (mst_window_inputs, mst_eval_accumulate)
// The two small launches that let a held-out round stay on the device: the K clips' small inputs gathered out of the song
// table by row indices read HERE (a captured launch serves other songs), and the batch folded into the round's 41 doubles.
// Both are latency-bound; what they owe is exactness: bit copies, one fixed summation order, no atomics.
#define WI_THREADS 256
#define WI_CHUNK 1024        // floats of a clip's concatenated fields one workgroup copies

struct WindowInputsArgs {
    int32_t n, src[MST_ROW_FIELDS], len[MST_ROW_FIELDS], at[MST_ROW_FIELDS + 1];     // at[f]: field f's first float in the concatenation
    int64_t dst[MST_ROW_FIELDS];
};

// workgroup b: chunk b % chunks of clip b / chunks.  The row index is one load per workgroup (every lane reads the same
// address); lanes stride over the chunk's floats.  Words are moved as uint32: a bit copy whatever the float holds.
__global__ __launch_bounds__(WI_THREADS) void window_inputs_kernel(const uint32_t* table, int table_rows, int row_floats, const int32_t* rows,
                                                                   int chunks, WindowInputsArgs a, int64_t clip_stride, uint32_t* ws) {
    const int k = blockIdx.x / chunks;
    const int c0 = (blockIdx.x % chunks) * WI_CHUNK;
    const int total = a.at[a.n];
    const int c1 = c0 + WI_CHUNK < total ? c0 + WI_CHUNK : total;
    const int row = MST_UNIFORM(rows[k]);
    const bool ok = row >= 0 && row < table_rows;               // a row outside the table is never read: quiet NaNs instead
    const uint32_t* src = table + (ok ? (int64_t)row * row_floats : 0);
    uint32_t* dst = ws + (int64_t)k * clip_stride;
    for (int e = c0 + (int)threadIdx.x; e < c1; e += WI_THREADS) {
        int f = 0;
        while (f + 1 < a.n && e >= a.at[f + 1]) ++f;
        const int i = e - a.at[f];
        dst[a.dst[f] + i] = ok ? src[a.src[f] + i] : 0x7fc00000u;
    }
}

extern "C" int32_t mst_window_inputs(const float* table, int32_t table_rows, int32_t row_floats, const int32_t* rows, int32_t n_clips,
                                     const mst_row_fields* fields, int64_t clip_stride, float* ws, mst_stream stream) {
    if (!table || !rows || !fields || !ws || n_clips < 1 || table_rows < 1 || row_floats < 1 || clip_stride < 0 ||
        fields->n < 1 || fields->n > MST_ROW_FIELDS || ((uintptr_t)table & 3) || ((uintptr_t)ws & 3))
        return MST_ERR_ARG;
    WindowInputsArgs a;
    a.n = fields->n;
    int64_t total = 0;
    for (int f = 0; f < MST_ROW_FIELDS; ++f) {
        const bool live = f < fields->n;
        if (live && (fields->src[f] < 0 || fields->len[f] < 0 || fields->dst[f] < 0 ||
                     (int64_t)fields->src[f] + fields->len[f] > row_floats))
            return MST_ERR_ARG;
        a.src[f] = live ? fields->src[f] : 0;
        a.len[f] = live ? fields->len[f] : 0;
        a.dst[f] = live ? fields->dst[f] : 0;
        a.at[f] = (int32_t)total;
        total += a.len[f];                                       // <= 8 * row_floats: may pass 2^31 only for a row of 2^28 floats
        if (total >= ((int64_t)1 << 31)) return MST_ERR_ARG;
    }
    a.at[MST_ROW_FIELDS] = (int32_t)total;
    for (int f = fields->n; f < MST_ROW_FIELDS; ++f) a.at[f] = (int32_t)total;
    if (total == 0) return MST_OK;                               // every named field is empty: nothing to write
    const int64_t chunks = (total + WI_CHUNK - 1) / WI_CHUNK;
    if (chunks * n_clips > 0x7fffffff) return MST_ERR_ARG;
    hipLaunchKernelGGL(window_inputs_kernel, dim3((unsigned)(chunks * n_clips)), dim3(WI_THREADS), 0, (hipStream_t)stream,
                       (const uint32_t*)table, (int)table_rows, (int)row_floats, rows, (int)chunks, a, clip_stride, (uint32_t*)ws);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

// One 64-lane workgroup; lane w < MST_EVAL_ACC_WORDS owns acc[w] and adds its terms left to right in float64, starting from the
// word's value on entry: clip 0, 1, ... and, for the pitched record, channel 0, 1, ... within a clip — the order of a host loop.
// The loads do not depend on the add chains, the adds do, so the two are separated: all 64 lanes copy the next stretch of the
// batch into LDS — plain consecutive addresses, EVAL_ACC_BATCH loads per lane in flight before the first is used — and the
// owning lanes then walk it in order.  First the loss rows (lanes 0..16), then the records (lanes 17..40); a stretch is as many
// whole loss rows, or whole records, as the 32 KB hold, so any n_clips and any channel count goes through the same code.
// (A lane per word that loaded its own terms from global memory took 46 to 58 us for 64 clips of 4 channels whatever its
// look-ahead: one wave issuing ~80 instructions of address arithmetic per term for the 256 terms of a pitched word.)
#define EVAL_ACC_LDS 4096            // doubles: 512 records, or 8192 floats
#define EVAL_ACC_BATCH 16
#define EVAL_ACC_WALK 8              // LDS reads a walking lane issues together; the adds behind them are selects, not branches

template <class V>
__device__ __forceinline__ void eval_acc_stage(V* dst, const V* src, int count) {
    for (int i0 = 0; i0 < count; i0 += 64 * EVAL_ACC_BATCH) {
        V r[EVAL_ACC_BATCH];
#pragma unroll
        for (int q = 0; q < EVAL_ACC_BATCH; ++q) {
            const int i = i0 + q * 64 + (int)threadIdx.x;
            r[q] = src[i < count ? i : count - 1];               // past the end: a valid address, the value is dropped
        }
#pragma unroll
        for (int q = 0; q < EVAL_ACC_BATCH; ++q) {
            const int i = i0 + q * 64 + (int)threadIdx.x;
            if (i < count) dst[i] = r[q];
        }
    }
}

__global__ __launch_bounds__(64) void eval_accumulate_kernel(const float* losses, const double* metrics, int n_clips, int channels,
                                                             const int32_t* live, double* acc) {
    __shared__ double sm[EVAL_ACC_LDS];
    float* sl = reinterpret_cast<float*>(sm);
    const int w = threadIdx.x;
    int n = live ? *live : n_clips;
    n = n < 0 ? 0 : (n > n_clips ? n_clips : n);
    if (n == 0) return;                                          // (every lane) acc + nothing: every word keeps its bits
    const bool owner = w < MST_EVAL_ACC_WORDS;
    const bool is_loss = w < 2 + MST_N_LOSSES;                   // [0], [1] and the leaf sums; the other owners hold record words
    double sum = owner ? acc[w] : 0.0;

    // ---- the loss rows: [0] and [1] count, [2 + i] adds leaf i
    const bool count = w < 2;
    const bool gated = w == 1 || (w >= 2 + MST_L_U_TOTAL && w <= 2 + MST_L_U_DURATION);     // only for clips with percussion
    const int leaf = is_loss && !count ? w - 2 : 0;
    const int rows_per = 2 * EVAL_ACC_LDS / MST_N_LOSSES;
    for (int k0 = 0; k0 < n; k0 += rows_per) {
        const int nk = n - k0 < rows_per ? n - k0 : rows_per;
        eval_acc_stage(sl, losses + (int64_t)k0 * MST_N_LOSSES, nk * MST_N_LOSSES);
        __syncthreads();
        if (is_loss) {
            for (int k1 = 0; k1 < nk; k1 += EVAL_ACC_WALK) {
                float u[EVAL_ACC_WALK], f[EVAL_ACC_WALK];
#pragma unroll
                for (int q = 0; q < EVAL_ACC_WALK; ++q) {
                    const int k = k1 + q < nk ? k1 + q : nk - 1;
                    u[q] = sl[k * MST_N_LOSSES + MST_L_U_TOTAL];
                    f[q] = sl[k * MST_N_LOSSES + leaf];
                }
#pragma unroll
                for (int q = 0; q < EVAL_ACC_WALK; ++q) {
                    const double next = sum + (count ? 1.0 : (double)f[q]);
                    // an absent unpitched leaf (NaN total: no percussion) is skipped, not added as 0
                    sum = k1 + q < nk && (!gated || u[q] == u[q]) ? next : sum;
                }
            }
        }
        __syncthreads();
    }

    // ---- the records: clip after clip `channels` pitched ones, the unpitched one, the song-info one
    const int per = channels + 2;
    const int m = is_loss ? 0 : w - 2 - MST_N_LOSSES;
    const int j = m % MST_METRIC_WORDS, which = m / MST_METRIC_WORDS;           // record word; 0 pitched, 1 unpitched, 2 song info
    const bool plus_one = which == 2 && j == MST_METRIC_WORDS - 1;              // the song-info record's last word counts the clips
    const int64_t records = (int64_t)n * per;
    const int recs_per = EVAL_ACC_LDS / MST_METRIC_WORDS;
    for (int64_t r0 = 0; r0 < records; r0 += recs_per) {
        const int nr = (int)(records - r0 < recs_per ? records - r0 : recs_per);
        eval_acc_stage(sm, metrics + r0 * MST_METRIC_WORDS, nr * MST_METRIC_WORDS);
        __syncthreads();
        if (owner && !is_loss) {
            int rr = (int)(r0 % per);                            // the stretch's first record within its clip: the same in every lane
            for (int r1 = 0; r1 < nr; r1 += EVAL_ACC_WALK) {
                double v[EVAL_ACC_WALK];
#pragma unroll
                for (int q = 0; q < EVAL_ACC_WALK; ++q) v[q] = sm[(r1 + q < nr ? r1 + q : nr - 1) * MST_METRIC_WORDS + j];
#pragma unroll
                for (int q = 0; q < EVAL_ACC_WALK; ++q) {
                    const int kind = rr < channels ? 0 : rr - channels + 1;
                    const double next = sum + (plus_one ? v[q] + 1.0 : v[q]);
                    sum = r1 + q < nr && kind == which ? next : sum;
                    rr = rr + 1 == per ? 0 : rr + 1;
                }
            }
        }
        __syncthreads();
    }
    if (owner) acc[w] = sum;
}

extern "C" int32_t mst_eval_accumulate(const float* losses, const double* metrics, int32_t n_clips, int32_t channels,
                                       const int32_t* live, double* acc, mst_stream stream) {
    if (!losses || !metrics || !acc || n_clips < 1 || channels < 1 || ((uintptr_t)metrics & 7) || ((uintptr_t)acc & 7) ||
        ((uintptr_t)losses & 3) || (int64_t)n_clips * channels >= ((int64_t)1 << 31))
        return MST_ERR_ARG;
    hipLaunchKernelGGL(eval_accumulate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, losses, metrics, (int)n_clips, (int)channels,
                       live, acc);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

// ------------------------------------------------------------------ batched style transfer (mst_clip_gather, mst_style_sums)
// The two small launches that let a style swap and its score stay on the device.  Like the windowed evaluation's they are
// latency-bound and owe exactness: a bit copy by a device index, and six left-to-right float64 sums per clip.
#define CG_THREADS 256
#define CG_CHUNK 1024        // floats of a clip one workgroup copies

// workgroup b: chunk b % chunks of clip b / chunks.  The index is one load per workgroup, as in window_inputs_kernel.
__global__ __launch_bounds__(CG_THREADS) void clip_gather_kernel(const uint32_t* src, int src_rows, int64_t src_stride, uint32_t* dst,
                                                                 int64_t dst_stride, const int32_t* idx, int chunks, int64_t len) {
    const int k = blockIdx.x / chunks;
    const int64_t c0 = (int64_t)(blockIdx.x % chunks) * CG_CHUNK;
    const int64_t c1 = c0 + CG_CHUNK < len ? c0 + CG_CHUNK : len;
    const int row = idx ? MST_UNIFORM(idx[k]) : k;
    const bool ok = row >= 0 && row < src_rows;                 // a row outside src is never read: quiet NaNs instead
    const uint32_t* from = src + (ok ? (int64_t)row * src_stride : 0);
    uint32_t* to = dst + (int64_t)k * dst_stride;
    for (int64_t i = c0 + threadIdx.x; i < c1; i += CG_THREADS) to[i] = ok ? from[i] : 0x7fc00000u;
}

// floats from the first to one past the last of `rows` runs of `len` floats, `stride` apart; false when that overflows
static bool span_floats(int64_t rows, int64_t stride, int64_t len, int64_t* span) {
    int64_t s;
    return !__builtin_mul_overflow(rows - 1, stride, &s) && !__builtin_add_overflow(s, len, span) && *span < ((int64_t)1 << 60);
}

extern "C" int32_t mst_clip_gather(const float* src, int32_t src_rows, int64_t src_stride, float* dst, int64_t dst_stride,
                                   const int32_t* idx, int32_t n_clips, int64_t len, mst_stream stream) {
    if (!src || !dst || n_clips < 1 || src_rows < 1 || len < 1 || src_stride < 0 || dst_stride < 0 || (dst_stride < len && n_clips > 1) ||
        ((uintptr_t)src & 3) || ((uintptr_t)dst & 3))
        return MST_ERR_ARG;
    int64_t src_span, dst_span;
    if (!span_floats(src_rows, src_stride, len, &src_span) || !span_floats(n_clips, dst_stride, len, &dst_span)) return MST_ERR_ARG;
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + 4 * (uintptr_t)src_span, d0 = (uintptr_t)dst, d1 = d0 + 4 * (uintptr_t)dst_span;
    if (s0 < d1 && d0 < s1) return MST_ERR_ARG;                 // a permutation in place is a race: go through a side buffer
    const int64_t chunks = (len + CG_CHUNK - 1) / CG_CHUNK;
    if (chunks * n_clips > 0x7fffffff) return MST_ERR_ARG;
    hipLaunchKernelGGL(clip_gather_kernel, dim3((unsigned)(chunks * n_clips)), dim3(CG_THREADS), 0, (hipStream_t)stream,
                       (const uint32_t*)src, (int)src_rows, src_stride, (uint32_t*)dst, dst_stride, idx, (int)chunks, len);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

// One 64-lane workgroup per clip; lane w < 6 owns word w and adds its products left to right in float64.  As in
// eval_accumulate_kernel the loads do not depend on the add chains: all 64 lanes copy the next stretch of x, y and z into LDS
// and the six owners then walk it in order.  The product of two floats widened to double is exact (48 significant bits, and no
// float product leaves double's range), so whether the compiler contracts the multiply and the add changes no bit.
#define SS_CHUNK 1024        // floats of each of the three vectors per stretch: 12 KB of LDS

__global__ __launch_bounds__(64) void style_sums_kernel(const float* a, int64_t a_stride, const float* b, int b_rows, int64_t b_stride,
                                                        const int32_t* idx, int64_t len, double* out) {
    __shared__ float sm[3][SS_CHUNK];
    const int k = blockIdx.x, w = threadIdx.x;
    const int row = idx ? MST_UNIFORM(idx[k]) : k;
    const bool y_ok = row >= 0 && row < b_rows, z_ok = k < b_rows;      // a row outside b is never read: its words are NaN
    const float* x = a + (int64_t)k * a_stride;
    const float* v[3] = {x, y_ok ? b + (int64_t)row * b_stride : x, z_ok ? b + (int64_t)k * b_stride : x};
    const int pa = (w == 0 || w == 3 || w == 4) ? 0 : (w == 1 || w == 5) ? 1 : 2;
    const int pb = w == 0 ? 0 : (w == 1 || w == 3) ? 1 : 2;
    double sum = 0.0;
    for (int64_t i0 = 0; i0 < len; i0 += SS_CHUNK) {                    // workgroup-uniform
        const int n = (int)(len - i0 < SS_CHUNK ? len - i0 : SS_CHUNK);
        for (int q = 0; q < 3; ++q)
            for (int i = w; i < n; i += 64) sm[q][i] = v[q][i0 + i];
        __syncthreads();
        if (w < 6) {
#pragma unroll 8
            for (int i = 0; i < n; ++i) sum += (double)sm[pa][i] * (double)sm[pb][i];
        }
        __syncthreads();                                                // sm is rewritten by the next stretch
    }
    const bool uses_y = w == 1 || w == 3 || w == 5, uses_z = w == 2 || w == 4 || w == 5;
    if ((uses_y && !y_ok) || (uses_z && !z_ok)) sum = __builtin_nan("");
    if (w < 6) out[(int64_t)k * 8 + w] = sum;
    if (w == 6) out[(int64_t)k * 8 + 6] = (double)len;
    if (w == 7) out[(int64_t)k * 8 + 7] = 0.0;
}

extern "C" int32_t mst_style_sums(const float* a, int64_t a_stride, const float* b, int32_t b_rows, int64_t b_stride, const int32_t* idx,
                                  int32_t n_clips, int64_t len, double* out, mst_stream stream) {
    if (!a || !b || !out || n_clips < 1 || b_rows < 1 || len < 1 || len >= ((int64_t)1 << 31) || a_stride < 0 || b_stride < 0 ||
        ((uintptr_t)a & 3) || ((uintptr_t)b & 3) || ((uintptr_t)out & 7))
        return MST_ERR_ARG;
    hipLaunchKernelGGL(style_sums_kernel, dim3((unsigned)n_clips), dim3(64), 0, (hipStream_t)stream, a, a_stride, b, (int)b_rows, b_stride,
                       idx, len, out);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

// ------------------------------------------------------------------ style bank (mst_style_put, mst_style_mix, mst_info_decide)
// The three small launches that let a style come from a bank of stored rows instead of another clip of the batch: a scatter of
// the batch's style slots into bank rows, a CSR-weighted sum of bank rows into the slots, and apply_style's host decisions (the
// top instruments, the mode, the tempo) taken where the predictions lie.  Like their neighbours they are latency-bound and owe
// exactness: a bit copy, one fixed order of separately rounded fp32 operations, one fixed ranking.

// workgroup b: chunk b % chunks of clip b / chunks, as clip_gather_kernel; a clip whose row is outside the bank writes nothing
__global__ __launch_bounds__(CG_THREADS) void style_put_kernel(const uint32_t* src, int64_t src_stride, uint32_t* bank, int bank_rows,
                                                               int64_t bank_stride, const int32_t* rows, int chunks, int64_t len) {
    const int k = blockIdx.x / chunks;
    const int row = MST_UNIFORM(rows[k]);
    if (row < 0 || row >= bank_rows) return;                    // (workgroup-uniform) how a padded batch's repeats are dropped
    const int64_t c0 = (int64_t)(blockIdx.x % chunks) * CG_CHUNK;
    const int64_t c1 = c0 + CG_CHUNK < len ? c0 + CG_CHUNK : len;
    const uint32_t* from = src + (int64_t)k * src_stride;
    uint32_t* to = bank + (int64_t)row * bank_stride;
    for (int64_t i = c0 + threadIdx.x; i < c1; i += CG_THREADS) to[i] = from[i];
}

// do [a, a + 4 * na) and [b, b + 4 * nb) intersect?
static bool floats_intersect(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + 4 * (uintptr_t)na, b0 = (uintptr_t)b, b1 = b0 + 4 * (uintptr_t)nb;
    return a0 < b1 && b0 < a1;
}

extern "C" int32_t mst_style_put(const float* src, int64_t src_stride, float* bank, int32_t bank_rows, int64_t bank_stride,
                                 const int32_t* rows, int32_t n_clips, int64_t len, mst_stream stream) {
    if (!src || !bank || !rows || n_clips < 1 || bank_rows < 1 || len < 1 || src_stride < 0 || bank_stride < 0 ||
        (bank_stride < len && bank_rows > 1) || ((uintptr_t)src & 3) || ((uintptr_t)bank & 3) || ((uintptr_t)rows & 3))
        return MST_ERR_ARG;
    int64_t src_span, bank_span;
    if (!span_floats(n_clips, src_stride, len, &src_span) || !span_floats(bank_rows, bank_stride, len, &bank_span)) return MST_ERR_ARG;
    if (floats_intersect(src, src_span, bank, bank_span)) return MST_ERR_ARG;
    const int64_t chunks = (len + CG_CHUNK - 1) / CG_CHUNK;
    if (chunks * n_clips > 0x7fffffff) return MST_ERR_ARG;
    hipLaunchKernelGGL(style_put_kernel, dim3((unsigned)(chunks * n_clips)), dim3(CG_THREADS), 0, (hipStream_t)stream,
                       (const uint32_t*)src, src_stride, (uint32_t*)bank, (int)bank_rows, bank_stride, rows, (int)chunks, len);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

// Workgroup b: chunk b % chunks (SM_CHUNK floats) of clip b / chunks; lane t owns floats [4 t, 4 t + 4) of the chunk and walks
// the clip's entries in order, so a float's chain is ((w0 x0) + w1 x1) + ... with every product and every sum rounded on its own
// (mul_rounded; the sum of an opaque product cannot contract).  The entries (idx, w) are staged through LDS SM_STAGE at a time
// with consecutive loads: the row loads then depend on LDS, not on a global load before them.  VEC: every row starts on a 16-byte
// boundary (bank and bank_stride say so), so a lane's four floats are one load; the ragged tail of a row and the unaligned case
// take scalar loads.  Only floats of named rows are read.  All loop bounds are workgroup-uniform.
#define SM_THREADS 256
#define SM_CHUNK (4 * SM_THREADS)
#define SM_STAGE 256

template <bool VEC>
__global__ __launch_bounds__(SM_THREADS) void style_mix_kernel(const float* bank, int bank_rows, int64_t bank_stride, const int32_t* offsets,
                                                               const int32_t* idx, const float* w, int n_entries, float* dst,
                                                               int64_t dst_stride, int chunks, int64_t len) {
    __shared__ int32_t s_idx[SM_STAGE];
    __shared__ float s_w[SM_STAGE];
    const int k = blockIdx.x / chunks, tid = threadIdx.x;
    const int64_t i0 = (int64_t)(blockIdx.x % chunks) * SM_CHUNK + 4 * tid;
    const int n = (int)(len - i0 >= 4 ? 4 : len - i0 > 0 ? len - i0 : 0);          // floats this lane owns
    const int e0 = MST_UNIFORM(offsets[k]), e1 = MST_UNIFORM(offsets[k + 1]);
    bool bad = e0 < 0 || e1 > n_entries || e1 <= e0;            // an empty, decreasing or outlying range: nothing is read
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const MST_GLOBAL_AS float* bg = (const MST_GLOBAL_AS float*)bank;
    if (!bad) {
        for (int s0 = e0; s0 < e1; s0 += SM_STAGE) {
            const int m = e1 - s0 < SM_STAGE ? e1 - s0 : SM_STAGE;
            if (tid < m) {
                s_idx[tid] = idx[s0 + tid];
                s_w[tid] = w[s0 + tid];
            }
            __syncthreads();
            for (int j = 0; j < m; ++j) {
                const int row = s_idx[j];
                const float wj = s_w[j];
                const bool ok = row >= 0 && row < bank_rows;    // a row outside the bank is never read: the clip becomes NaN
                bad |= !ok;
                const MST_GLOBAL_AS float* x = bg + ((ok ? (int64_t)row * bank_stride : 0) + i0);
                float v[4] = {0.f, 0.f, 0.f, 0.f};
                if (VEC && n == 4) {
                    const roll_f4 q = *reinterpret_cast<const MST_GLOBAL_AS roll_f4*>(x);
                    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (c < n) v[c] = x[c];
                }
                const bool first = s0 == e0 && j == 0;          // the first product is not added to a zero
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float p = mul_rounded(wj, v[c]);
                    acc[c] = first ? p : acc[c] + p;
                }
            }
            __syncthreads();                                    // the stage is rewritten by the next stretch
        }
    }
    float* to = dst + (int64_t)k * dst_stride + i0;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (c < n) to[c] = bad ? __uint_as_float(0x7fc00000u) : acc[c];
}

extern "C" int32_t mst_style_mix(const float* bank, int32_t bank_rows, int64_t bank_stride, const int32_t* offsets, const int32_t* idx,
                                 const float* w, int32_t n_entries, float* dst, int64_t dst_stride, int32_t n_clips, int64_t len,
                                 mst_stream stream) {
    if (!bank || !offsets || !idx || !w || !dst || n_clips < 1 || bank_rows < 1 || n_entries < 1 || len < 1 || bank_stride < 0 ||
        dst_stride < 0 || (dst_stride < len && n_clips > 1) || ((uintptr_t)bank & 3) || ((uintptr_t)dst & 3) || ((uintptr_t)offsets & 3) ||
        ((uintptr_t)idx & 3) || ((uintptr_t)w & 3))
        return MST_ERR_ARG;
    int64_t bank_span, dst_span;
    if (!span_floats(bank_rows, bank_stride, len, &bank_span) || !span_floats(n_clips, dst_stride, len, &dst_span)) return MST_ERR_ARG;
    if (floats_intersect(bank, bank_span, dst, dst_span)) return MST_ERR_ARG;
    const int64_t chunks = (len + SM_CHUNK - 1) / SM_CHUNK;
    if (chunks * n_clips > 0x7fffffff) return MST_ERR_ARG;
    const dim3 grid((unsigned)(chunks * n_clips)), block(SM_THREADS);
    if (!((uintptr_t)bank & 15) && bank_stride % 4 == 0)
        hipLaunchKernelGGL(style_mix_kernel<true>, grid, block, 0, (hipStream_t)stream, bank, (int)bank_rows, bank_stride, offsets, idx, w,
                           (int)n_entries, dst, dst_stride, (int)chunks, len);
    else
        hipLaunchKernelGGL(style_mix_kernel<false>, grid, block, 0, (hipStream_t)stream, bank, (int)bank_rows, bank_stride, offsets, idx, w,
                           (int)n_entries, dst, dst_stride, (int)chunks, len);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

// One 64-lane workgroup (one wave) per clip; lane j < n_logits owns logit j.  The ranking is a counting rank: lane j counts the
// logits that come before its own — a loop of n_logits comparisons whatever the values — and the order is total (descending;
// equal values by index; a NaN after every number, NaNs by index), so the ranks are a permutation of 0 .. n_logits - 1.  Pooled:
// every workgroup first sums the live clips' predictions itself, left to right in clip order (no workgroup waits for another),
// and all take the one decision.
struct InfoDecideArgs {
    int32_t n_logits, n_groups, channels, pool, n_clips;
    int8_t group_of[MST_DECIDE_MAX_LOGITS];
};

__global__ __launch_bounds__(64) void info_decide_kernel(const float* logits, const float* mode_pred, const float* bpm_pred,
                                                         int64_t pred_stride, InfoDecideArgs a, const int32_t* live, float* instr,
                                                         float* mode, float* bpm, int64_t out_stride, int32_t* decisions) {
    __shared__ float s_x[64];
    __shared__ int s_rank[64];
    __shared__ int s_pick[64];
    const int k = blockIdx.x, j = threadIdx.x, NL = a.n_logits, P = NL - 1;
    float x = 0.f, m0, m1, b;
    if (a.pool) {
        int n = live ? MST_UNIFORM(live[0]) : a.n_clips;
        n = n < 1 ? 1 : n > a.n_clips ? a.n_clips : n;
        m0 = mode_pred[0], m1 = mode_pred[1], b = bpm_pred[0];
        if (j < NL) x = logits[j];
        for (int c = 1; c < n; ++c) {                           // (workgroup-uniform)
            const int64_t at = (int64_t)c * pred_stride;
            if (j < NL) x = x + logits[at + j];
            m0 = m0 + mode_pred[at], m1 = m1 + mode_pred[at + 1], b = b + bpm_pred[at];
        }
        b = b / (float)n;
    } else {
        const int64_t at = (int64_t)k * pred_stride;
        if (j < NL) x = logits[at + j];
        m0 = mode_pred[at], m1 = mode_pred[at + 1], b = bpm_pred[at];
    }
    s_x[j] = x;
    __syncthreads();
    int rank = 0;
    const bool nan_j = x != x;
    for (int i = 0; i < NL; ++i) {
        const float y = s_x[i];
        const bool nan_i = y != y;
        const bool before = nan_i ? (nan_j && i < j) : (nan_j || y > x || (y == x && i < j));
        rank += before ? 1 : 0;
    }
    s_rank[j] = rank;
    __syncthreads();
    const int perc = s_rank[P];
    if (j < P) {
        const int pitched_rank = rank - (perc < rank ? 1 : 0);  // its rank among the pitched instruments
        if (pitched_rank < a.channels) s_pick[pitched_rank] = j;
    }
    __syncthreads();
    const int row = P + a.n_groups;
    float* out = instr + (int64_t)k * out_stride;
    for (int e = j; e < a.channels * row; e += 64) {
        const int c = e / row, f = e - c * row, pick = s_pick[c];
        out[e] = (f < P ? f == pick : f - P == (int)a.group_of[pick]) ? 1.f : 0.f;
    }
    const int major_or_minor = m1 > m0 ? 1 : 0;                 // the first index of the larger logit
    int32_t* rec = decisions + (int64_t)k * (a.channels + 2);
    if (j < a.channels) rec[j] = s_pick[j];
    if (j == 0) {
        rec[a.channels] = perc;
        rec[a.channels + 1] = major_or_minor;
        mode[(int64_t)k * out_stride] = major_or_minor ? 0.f : 1.f;
        mode[(int64_t)k * out_stride + 1] = major_or_minor ? 1.f : 0.f;
        bpm[(int64_t)k * out_stride] = rintf(b);
    }
}

extern "C" int32_t mst_info_decide(const float* instruments_pred, const float* mode_pred, const float* bpm_pred, int64_t pred_stride,
                                   int32_t n_logits, const int32_t* group_of, int32_t n_groups, int32_t channels, int32_t n_clips,
                                   int32_t pool, const int32_t* live, float* instr, float* mode, float* bpm, int64_t out_stride,
                                   int32_t* decisions, mst_stream stream) {
    if (!instruments_pred || !mode_pred || !bpm_pred || !group_of || !instr || !mode || !bpm || !decisions || n_clips < 1 ||
        n_logits < 2 || n_logits > MST_DECIDE_MAX_LOGITS || n_groups < 1 || n_groups > 127 || channels < 1 || channels > n_logits - 1 ||
        pred_stride < 0 || out_stride < 0)
        return MST_ERR_ARG;
    const void* all[] = {instruments_pred, mode_pred, bpm_pred, instr, mode, bpm, decisions, live};
    for (const void* p : all)
        if ((uintptr_t)p & 3) return MST_ERR_ARG;
    // a clip's three results may not lie on its three predictions or on one another (the runs of clip 0 stand for all: the
    // strides are shared)
    const int64_t row = (int64_t)(n_logits - 1 + n_groups) * channels;
    const void* runs[] = {instr, mode, bpm, instruments_pred, mode_pred, bpm_pred};
    const int64_t lens[] = {row, 2, 1, n_logits, 2, 1};
    for (int p = 0; p < 3; ++p)
        for (int q = p + 1; q < 6; ++q)
            if (floats_intersect(runs[p], lens[p], runs[q], lens[q])) return MST_ERR_ARG;
    if (n_clips > 1 && out_stride < row) return MST_ERR_ARG;     // the clips' instrument rows would overlap
    InfoDecideArgs a;
    a.n_logits = n_logits, a.n_groups = n_groups, a.channels = channels, a.pool = pool != 0, a.n_clips = n_clips;
    for (int i = 0; i < MST_DECIDE_MAX_LOGITS; ++i) a.group_of[i] = 0;
    for (int i = 0; i < n_logits - 1; ++i) {
        if (group_of[i] < 0 || group_of[i] >= n_groups) return MST_ERR_ARG;
        a.group_of[i] = (int8_t)group_of[i];
    }
    hipLaunchKernelGGL(info_decide_kernel, dim3((unsigned)n_clips), dim3(64), 0, (hipStream_t)stream, instruments_pred, mode_pred, bpm_pred,
                       pred_stride, a, live, instr, mode, bpm, out_stride, decisions);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

// ------------------------------------------------------------------ style search (mst_style_search)
// Which rows of a bank resemble a style: the cosines of a batch of queries against every row and the k best per query, in two
// launches.  (a) One workgroup per SS_SLAB rows and SS_QT queries: k-tiles of SS_KT floats of both are staged in LDS (the bank is
// read once per query tile), wave w owns rows [16 w, 16 w + 16) of the slab against all SS_QT queries, four 16x16x4 f32 MFMA
// accumulators, every k-tile visited in order — one fmaf chain per (query, row), no k-split; the norms are the same chain walked
// by one lane per row over the staged values.  Zeros staged behind `len` add nothing to a chain (fmaf(0, 0, acc) = acc for the
// acc >= +0 of a norm and for every acc of a dot but a -0 that only an underflowed product can leave).  The scores then go
// through LDS to a counting rank per query — lane = row, 64 comparisons whatever the values, a total order — and the slab's k best
// go to scratch.  (b) One workgroup per query picks the best candidate below the previous pick, k times.
// No atomics, no workgroup waits for another.
#define SS_THREADS 256
#define SS_SLAB MST_SEARCH_SLAB
#define SS_QT 64             // queries of a workgroup
#define SS_KT 32             // floats of a k-tile
#define SS_LD (SS_KT + 4)    // row stride of a staged tile: lane l reads [l & 15][4 kk + (l >> 4)], 36 r + c hits 64 different banks
#define SS_SD (SS_SLAB + 4)  // row stride of the score image
static_assert(SS_SLAB == 64 && SS_QT == 64 && SS_THREADS == 256, "style_search_kernel: one lane per row, 16 rows per wave");

typedef uint32_t ss_u4 __attribute__((ext_vector_type(4)));

// the order of the ranking as unsigned integers: larger = earlier.  0 is no float's key (the smallest is -inf's, 0x007fffff),
// so it marks a row that is not rankable; -0 and +0 are one key, as they are equal as floats.
__device__ __forceinline__ uint32_t search_key(float score, int order) {
    uint32_t u = __float_as_uint(order > 0 ? score : -score);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// this lane's two 16-byte pieces of a 64 x SS_KT tile of rows [first, first + n_rows) of `base`, floats [i0, i0 + SS_KT): piece
// s = tid + 256 h is floats [4 (s & 7), + 4) of row s >> 3.  Nothing outside the rows' `len` floats is read: zeros instead.
template <bool VEC>
__device__ __forceinline__ void search_fetch(const float* base, int64_t stride, int64_t first, int n_rows, int i0, int len, int tid,
                                             roll_f4 (&v)[2]) {
    const MST_GLOBAL_AS float* g = (const MST_GLOBAL_AS float*)base;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int s = tid + SS_THREADS * h, r = s >> 3, i = i0 + 4 * (s & 7);
        roll_f4 x = {0.f, 0.f, 0.f, 0.f};
        if (r < n_rows && i < len) {
            const MST_GLOBAL_AS float* p = g + ((first + r) * stride + i);
            if (VEC && i + 4 <= len) {
                x = *reinterpret_cast<const MST_GLOBAL_AS roll_f4*>(p);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (i + c < len) x[c] = p[c];
            }
        }
        v[h] = x;
    }
}

__device__ __forceinline__ void search_stage(float* tile, int tid, const roll_f4 (&v)[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int s = tid + SS_THREADS * h;
        *reinterpret_cast<roll_f4*>(tile + (s >> 3) * SS_LD + 4 * (s & 7)) = v[h];
    }
}

template <bool VB, bool VQ>
__global__ __launch_bounds__(SS_THREADS) void style_search_kernel(const float* bank, int bank_rows, int64_t bank_stride, const int32_t* n_live,
                                                                  const int32_t* groups, const float* queries, int n_queries,
                                                                  int64_t query_stride, const int32_t* exclude, int len, int k, int order,
                                                                  int slabs, float* sc_scores, int32_t* sc_rows) {
    // the two staged tiles (2 x 64 x SS_LD floats) while the scores are summed, then the keys and the scores (2 x 64 x SS_SD)
    __shared__ __attribute__((aligned(16))) float sm[2 * SS_QT * SS_SD];
    __shared__ float s_nr[SS_SLAB], s_nq[SS_QT];
    __shared__ int32_t s_grp[SS_SLAB], s_ex[SS_QT];
    float* t_r = sm;
    float* t_q = sm + SS_SLAB * SS_LD;
    uint32_t* s_key = reinterpret_cast<uint32_t*>(sm);
    float* s_sc = sm + SS_QT * SS_SD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slab = blockIdx.x % slabs, q0 = (blockIdx.x / slabs) * SS_QT;
    const int row0 = slab * SS_SLAB;
    const int nq = n_queries - q0 < SS_QT ? n_queries - q0 : SS_QT;
    const int nr = bank_rows - row0 < SS_SLAB ? bank_rows - row0 : SS_SLAB;
    int live = n_live ? MST_UNIFORM(n_live[0]) : bank_rows;
    live = live < 0 ? 0 : live > bank_rows ? bank_rows : live;
    if (row0 >= live) {                                         // (workgroup-uniform) a slab behind the live rows is not read
        for (int e = tid; e < nq * k; e += SS_THREADS) {
            const int64_t at = ((int64_t)(q0 + e / k) * slabs + slab) * k + e % k;
            sc_rows[at] = -1;
            sc_scores[at] = __uint_as_float(0x7fc00000u);
        }
        return;
    }
    if (tid < SS_SLAB) s_grp[tid] = (groups && tid < nr) ? groups[row0 + tid] : -1;
    else if (tid < SS_SLAB + SS_QT) s_ex[tid - SS_SLAB] = (groups && exclude && tid - SS_SLAB < nq) ? exclude[q0 + tid - SS_SLAB] : -1;

    roll_f4 acc[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[n] = roll_f4{0.f, 0.f, 0.f, 0.f};
    float norm = 0.f;                                           // tid < 64: of row tid; tid < 128: of query tid - 64
    const float* n_at = tid < SS_SLAB ? t_r + tid * SS_LD : t_q + (tid - SS_SLAB) * SS_LD;
    const float* a_at = t_r + (wave * 16 + (lane & 15)) * SS_LD + (lane >> 4);
    const float* b_at = t_q + (lane & 15) * SS_LD + (lane >> 4);
    roll_f4 vr[2], vq[2];
    search_fetch<VB>(bank, bank_stride, row0, nr, 0, len, tid, vr);
    search_fetch<VQ>(queries, query_stride, q0, nq, 0, len, tid, vq);
    for (int i0 = 0; i0 < len; i0 += SS_KT) {                   // (workgroup-uniform)
        search_stage(t_r, tid, vr);
        search_stage(t_q, tid, vq);
        __syncthreads();
        if (i0 + SS_KT < len) {                                 // the next k-tile travels while this one is summed
            search_fetch<VB>(bank, bank_stride, row0, nr, i0 + SS_KT, len, tid, vr);
            search_fetch<VQ>(queries, query_stride, q0, nq, i0 + SS_KT, len, tid, vq);
        }
        if (tid < SS_SLAB + SS_QT) {
#pragma unroll
            for (int i4 = 0; i4 < SS_KT / 4; ++i4) {
                const roll_f4 x = *reinterpret_cast<const roll_f4*>(n_at + 4 * i4);
#pragma unroll
                for (int c = 0; c < 4; ++c) norm = __builtin_fmaf(x[c], x[c], norm);
            }
        }
#pragma unroll
        for (int kk = 0; kk < SS_KT / 4; ++kk) {
            const float a = a_at[4 * kk];
#pragma unroll
            for (int n = 0; n < 4; ++n)
                if (n * 16 < nq)                                // (workgroup-uniform)
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b_at[n * 16 * SS_LD + 4 * kk], acc[n], 0, 0, 0);
        }
        __syncthreads();                                        // the tiles are rewritten by the next stretch, or by the keys
    }
    if (tid < SS_SLAB) s_nr[tid] = norm;
    else if (tid < SS_SLAB + SS_QT) s_nq[tid - SS_SLAB] = norm;
    __syncthreads();
    // D[row = 4 (lane >> 4) + j][col = lane & 15] of accumulator n is (row 16 wave + ..., query 16 n + col)
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int q = n * 16 + (lane & 15);
        const float root_q = sqrtf(s_nq[q]);
        const int ex = s_ex[q];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = wave * 16 + (lane >> 4) * 4 + j;
            const float root_r = sqrtf(s_nr[r]);
            const float den = root_q * root_r;
            const float score = acc[n][j] / den;
            const bool rankable = row0 + r < live && !(ex >= 0 && s_grp[r] == ex) && score == score;
            s_key[q * SS_SD + r] = rankable ? search_key(score, order) : 0u;
            s_sc[q * SS_SD + r] = score;
        }
    }
    __syncthreads();
    // wave w ranks queries [16 w, 16 w + 16); lane = row.  (key, row) is different for every lane, so the ranks are a permutation
    // of 0 .. 63 and every position below k has exactly one writer: a rankable row, or -1 / NaN from one that is not.
    for (int qq = 0; qq < 16; ++qq) {
        const int q = wave * 16 + qq;
        if (q >= nq) break;                                     // (wave-uniform)
        const uint32_t own = s_key[q * SS_SD + lane];
        int rank = 0;
#pragma unroll
        for (int i4 = 0; i4 < SS_SLAB / 4; ++i4) {
            const ss_u4 o = *reinterpret_cast<const ss_u4*>(s_key + q * SS_SD + 4 * i4);
#pragma unroll
            for (int c = 0; c < 4; ++c) rank += (o[c] > own || (o[c] == own && 4 * i4 + c < lane)) ? 1 : 0;
        }
        if (rank < k) {
            const int64_t at = ((int64_t)(q0 + q) * slabs + slab) * k + rank;
            sc_rows[at] = own ? row0 + lane : -1;
            sc_scores[at] = own ? s_sc[q * SS_SD + lane] : __uint_as_float(0x7fc00000u);
        }
    }
}

// One workgroup per query over its m = slabs x k candidates: pick j is the largest (key, lowest row) below pick j - 1.  The
// 64-bit keys of rankable candidates are all different (the rows are), so "below the previous" removes exactly the picks made.
__global__ __launch_bounds__(SS_THREADS) void style_search_merge_kernel(const float* sc_scores, const int32_t* sc_rows, int m, int k, int order,
                                                                        int32_t* rows, float* scores) {
    __shared__ uint64_t s_best[SS_THREADS];
    const int tid = threadIdx.x, q = blockIdx.x;
    const int64_t base = (int64_t)q * m;
    uint64_t prev = ~(uint64_t)0;
    for (int j = 0; j < k; ++j) {                               // (workgroup-uniform)
        uint64_t best = 0;
        float best_score = 0.f;
        for (int c = tid; c < m; c += SS_THREADS) {
            const int32_t r = sc_rows[base + c];
            if (r < 0) continue;
            const float s = sc_scores[base + c];
            const uint64_t key = ((uint64_t)search_key(s, order) << 32) | (uint32_t)(0x7fffffff - r);
            if (key < prev && key > best) best = key, best_score = s;
        }
        s_best[tid] = best;
        __syncthreads();
        for (int s = SS_THREADS / 2; s > 0; s >>= 1) {
            if (tid < s && s_best[tid + s] > s_best[tid]) s_best[tid] = s_best[tid + s];
            __syncthreads();
        }
        const uint64_t win = s_best[0];
        __syncthreads();                                        // s_best is rewritten by the next pick
        if (win == 0) {
            if (tid == 0) {
                rows[(int64_t)q * k + j] = -1;
                scores[(int64_t)q * k + j] = __uint_as_float(0x7fc00000u);
            }
        } else if (best == win) {
            rows[(int64_t)q * k + j] = 0x7fffffff - (int32_t)(uint32_t)win;
            scores[(int64_t)q * k + j] = best_score;
        }
        prev = win;
    }
}

extern "C" int64_t mst_style_search_scratch_bytes(int32_t bank_rows, int32_t n_queries, int32_t k) {
    if (bank_rows < 1 || n_queries < 1 || n_queries > 4096 || k < 1 || k > MST_SEARCH_MAX_K) return 0;
    const int64_t slabs = ((int64_t)bank_rows + SS_SLAB - 1) / SS_SLAB;
    return 8 * slabs * n_queries * k;
}

extern "C" int32_t mst_style_search(const float* bank, int32_t bank_rows, int64_t bank_stride, const int32_t* n_live, const int32_t* groups,
                                    const float* queries, int32_t n_queries, int64_t query_stride, const int32_t* exclude, int64_t len,
                                    int32_t k, int32_t order, int32_t* rows, float* scores, void* scratch, mst_stream stream) {
    if (!bank || !queries || !rows || !scores || !scratch || bank_rows < 1 || n_queries < 1 || n_queries > 4096 || len < 1 || len > 4096 ||
        k < 1 || k > MST_SEARCH_MAX_K || (order != 1 && order != -1) || bank_stride < 0 || query_stride < 0 || (exclude && !groups) ||
        ((uintptr_t)scratch & 7))
        return MST_ERR_ARG;
    const void* all[] = {bank, queries, rows, scores, n_live, groups, exclude};
    for (const void* p : all)
        if ((uintptr_t)p & 3) return MST_ERR_ARG;
    int64_t bank_span, query_span;
    if (!span_floats(bank_rows, bank_stride, len, &bank_span) || !span_floats(n_queries, query_stride, len, &query_span)) return MST_ERR_ARG;
    const int64_t out = (int64_t)n_queries * k;
    if (floats_intersect(rows, out, scores, out) || floats_intersect(rows, out, bank, bank_span) || floats_intersect(rows, out, queries, query_span) ||
        floats_intersect(scores, out, bank, bank_span) || floats_intersect(scores, out, queries, query_span))
        return MST_ERR_ARG;
    const int64_t slabs = ((int64_t)bank_rows + SS_SLAB - 1) / SS_SLAB, tiles = (n_queries + SS_QT - 1) / SS_QT;
    if (slabs * tiles > 0x7fffffff) return MST_ERR_ARG;
    float* sc_scores = (float*)scratch;
    int32_t* sc_rows = (int32_t*)(sc_scores + slabs * n_queries * k);
    const dim3 grid((unsigned)(slabs * tiles)), block(SS_THREADS);
    const bool vb = !((uintptr_t)bank & 15) && bank_stride % 4 == 0, vq = !((uintptr_t)queries & 15) && query_stride % 4 == 0;
#define SS_LAUNCH(VB, VQ)                                                                                                              \
    hipLaunchKernelGGL((style_search_kernel<VB, VQ>), grid, block, 0, (hipStream_t)stream, bank, (int)bank_rows, bank_stride, n_live, groups, \
                       queries, (int)n_queries, query_stride, exclude, (int)len, (int)k, (int)order, (int)slabs, sc_scores, sc_rows)
    if (vb && vq) SS_LAUNCH(true, true);
    else if (vb) SS_LAUNCH(true, false);
    else if (vq) SS_LAUNCH(false, true);
    else SS_LAUNCH(false, false);
#undef SS_LAUNCH
    if (hipGetLastError() != hipSuccess) return MST_ERR_LAUNCH;
    hipLaunchKernelGGL(style_search_merge_kernel, dim3((unsigned)n_queries), block, 0, (hipStream_t)stream, sc_scores, sc_rows,
                       (int)(slabs * k), (int)k, (int)order, rows, scores);
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}
