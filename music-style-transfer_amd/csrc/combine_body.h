// Device bodies of the combine kernels (combine.hip has the maths), shared by the stand-alone kernels of combine.hip and by
// gemm_kernel, whose launch carries the combine steps of its dependency level (gemm.hip).
// A body is run by one 256-lane group: `t` is the lane's index inside the group, `blk` the group's index among the site's nblk.
// Every lane of the workgroup calls the body and reaches its barriers; `live` = false (a rider group behind the site's last, the
// lanes >= 256 of a small site's rider block) makes a lane neither load nor store.  part / red ...: the group's own LDS slices.
// MC: compile-time bound on the channel count (4: every site of the model up to 4 channels; COMBINE_MAXC: the general case).
// U grid-stride trips are processed together: every address first, then all U x MC loads (unconditional, through global-address
// pointers, with clamped element and channel indices), then the uses, predicated.  One memory round trip per group of trips
// instead of one per channel and trip.  Per lane and channel the elements are still accumulated in ascending order.
#pragma once
#include "mst_common.h"

typedef const MST_GLOBAL_AS float* comb_gptr;
template <int MC> struct CombineTrips { static constexpr int U = MC <= 4 ? 4 : 1; };

// sums `nv` per-lane values across the 256-lane group; result for value v lands in red[v]
template <int MC = COMBINE_MAXC>
__device__ __forceinline__ void block_sum_multi(float* vals, int nv, float (*part)[COMBINE_MAXC + 1], float* red, const int t, const bool live = true) {
    const int lane = t & 63, wv = t >> 6;
#pragma unroll
    for (int v = 0; v <= MC; ++v) {                 // static indices keep vals[] in registers; nv is workgroup-uniform
        // (MC <= 4: no branch around the few absent values' shuffles — a load that feeds vals[v] would be sunk into it)
        if (MC <= 4 || v < nv) {
            float x = vals[v];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
            if (lane == 0 && live && v < nv) part[wv][v] = x;
        }
    }
    __syncthreads();
    if (t < nv && live) red[t] = (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]);
    __syncthreads();
}

// element e of a rows x cols slice with row stride ld (32-bit index math: a slice has < 2^31 elements)
__device__ __forceinline__ int64_t elem_off(const CombineDesc& d, int e) {
    const unsigned r = (unsigned)e / (unsigned)d.cols;
    return (int64_t)r * d.ld + (int)((unsigned)e - r * (unsigned)d.cols);
}

// a site whose step one 256-lane group runs whole (reduction and elementwise pass): no cross-workgroup re-sum
__device__ __forceinline__ bool combine_site_small(const CombineDesc& d) { return (int64_t)d.rows * d.cols <= COMBINE_SMALL; }

// the x values of U trips from element e0 on, `stride` elements apart: v[u][c] = x_c[e0 + u * stride] (clamped to element 0 /
// channel 0 where there is none: the caller predicates the use); eo[u] = the element's offset inside a slice
template <int MC, int U>
__device__ __forceinline__ void combine_load_x(const CombineDesc& d, comb_gptr x, const unsigned e0, const unsigned stride, const unsigned n,
                                               float (&v)[U][MC], int64_t (&eo)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned e = e0 + u * stride;
        eo[u] = elem_off(d, e < n ? (int)e : 0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int c = 0; c < MC; ++c) {
            if (MC <= 4) v[u][c] = x[(int64_t)(c < d.Cn ? c : 0) * d.cs + eo[u]];
            else v[u][c] = c < d.Cn ? x[(int64_t)c * d.cs + eo[u]] : 0.f;      // (32 channels: the absent ones are not worth a load)
        }
    }
}

// part[blk*(MAXC+1) + c] = partial sum of squares of slice c over this group's elements
template <int MC>
__device__ __forceinline__ void combine_sumsq_body(const CombineDesc& d, const int blk, const int t, const bool live, const Bases& b,
                                                   float (*part)[COMBINE_MAXC + 1], float* red) {
    constexpr int U = CombineTrips<MC>::U;
    comb_gptr x = (comb_gptr)b.p[SP_WS] + d.x_off;
    const unsigned n = live ? (unsigned)(d.rows * d.cols) : 0u, stride = (unsigned)d.nblk * 256u;
    float acc[MC + 1];
#pragma unroll
    for (int c = 0; c <= MC; ++c) acc[c] = 0.f;
    for (unsigned e0 = (unsigned)blk * 256u + t; e0 < n; e0 += stride * U) {
        float v[U][MC];
        int64_t eo[U];
        combine_load_x<MC, U>(d, x, e0, stride, n, v, eo);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool ok = e0 + u * stride < n;     // a select, not a branch: a branch would take the trip's loads with it
#pragma unroll
            for (int c = 0; c < MC; ++c) acc[c] = (ok && c < d.Cn) ? fmaf(v[u][c], v[u][c], acc[c]) : acc[c];
        }
    }
    block_sum_multi<MC>(acc, d.Cn, part, red, t, live);
    if (live && t < d.Cn) b.p[SP_TMP][d.part_off + blk * (COMBINE_MAXC + 1) + t] = red[t];
}

// the norms n_c = sqrt(1 + sum of squares) and S = their sum in channel order, from the reduced sums in LDS: every lane computes
// them itself (a few square roots) instead of one lane writing them back for the others behind two more barriers
template <int MC>
__device__ __forceinline__ void combine_norms(const CombineDesc& d, const float* red, float (&nc)[MC], float& S) {
    S = 0.f;
#pragma unroll
    for (int c = 0; c < MC; ++c) {
        nc[c] = c < d.Cn ? sqrtf(1.f + red[c]) : 0.f;
        if (c < d.Cn) S += nc[c];
    }
}

// the per-workgroup partials of lane k < nblk, all loaded before the first use: vals[c] = partial c of workgroup t (nv values)
template <int MC>
__device__ __forceinline__ void combine_load_partials(const CombineDesc& d, comb_gptr tmp, const int t, const int nv, float (&vals)[MC + 1]) {
    comb_gptr p = tmp + d.part_off + (t < d.nblk ? t : 0) * (COMBINE_MAXC + 1);
#pragma unroll
    for (int c = 0; c <= MC; ++c) {
        if (MC <= 4) vals[c] = p[c < nv ? c : 0];
        else vals[c] = c < nv ? p[c] : 0.f;
    }
#pragma unroll
    for (int c = 0; c <= MC; ++c) vals[c] = (c < nv && t < d.nblk) ? vals[c] : 0.f;
}

// norms from the partials, then out = sum_c x_c n_c / S
template <int MC>
__device__ __forceinline__ void combine_apply_body(const CombineDesc& d, const int blk, const int t, const Bases& b,
                                                   float (*part)[COMBINE_MAXC + 1], float* red) {
    constexpr int U = CombineTrips<MC>::U;
    float* ws = b.p[SP_WS];
    float* tmp = b.p[SP_TMP];
    comb_gptr x = (comb_gptr)ws + d.x_off;
    const unsigned n = (unsigned)(d.rows * d.cols), stride = (unsigned)d.nblk * 256u;
    unsigned e0 = (unsigned)blk * 256u + t;
    float v[U][MC];
    int64_t eo[U];
    {   // re-sum the per-workgroup partials: lane k takes partial k, then a fixed-order tree (nblk <= 256); the first group of
        // trips is loaded in front of it and lands under the reduction
        float vals[MC + 1];
        combine_load_x<MC, U>(d, x, e0, stride, n, v, eo);
        combine_load_partials<MC>(d, (comb_gptr)tmp, t, d.Cn, vals);
        MST_SCHED_FENCE();       // (the scheduler otherwise starts the reduction, and waits, in front of the x loads)
        block_sum_multi<MC>(vals, d.Cn, part, red, t);
    }
    float nc[MC], S;
    combine_norms<MC>(d, red, nc, S);
    if (blk == 0 && t <= d.Cn) tmp[d.stats_off + t] = t < d.Cn ? sqrtf(1.f + red[t]) : S;
    while (e0 < n) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned e = e0 + u * stride;
            float a = 0.f;
#pragma unroll
            for (int c = 0; c < MC; ++c) if (c < d.Cn) a += v[u][c] * nc[c];
            if (e < n) ws[d.out_off + e] = a / S;
        }
        e0 += stride * U;
        if (e0 < n) combine_load_x<MC, U>(d, x, e0, stride, n, v, eo);
    }
}

// part[blk*(MAXC+1) + c] = partial a_c, part[blk*(MAXC+1) + Cn] = partial b
template <int MC>
__device__ __forceinline__ void combine_bwd_reduce_body(const CombineDesc& d, const int blk, const int t, const bool live, const Bases& b,
                                                        float (*part)[COMBINE_MAXC + 1], float* red) {
    constexpr int U = CombineTrips<MC>::U;
    comb_gptr x = (comb_gptr)b.p[SP_WS] + d.x_off;
    comb_gptr out = (comb_gptr)b.p[SP_WS] + d.out_off;
    comb_gptr go = (comb_gptr)b.p[SP_GRAD] + d.gout_off;
    const unsigned n = live ? (unsigned)(d.rows * d.cols) : 0u, stride = (unsigned)d.nblk * 256u;
    float acc[MC + 1];
#pragma unroll
    for (int c = 0; c <= MC; ++c) acc[c] = 0.f;
    for (unsigned e0 = (unsigned)blk * 256u + t; e0 < n; e0 += stride * U) {
        float v[U][MC], g[U], o[U];
        int64_t eo[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned e = e0 + u * stride, ec = e < n ? e : 0u;
            g[u] = go[ec];
            o[u] = out[ec];
        }
        combine_load_x<MC, U>(d, x, e0, stride, n, v, eo);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool ok = e0 + u * stride < n;
#pragma unroll
            for (int c = 0; c < MC; ++c) acc[c] = (ok && c < d.Cn) ? fmaf(g[u], v[u][c], acc[c]) : acc[c];
            acc[MC] = ok ? fmaf(g[u], o[u], acc[MC]) : acc[MC];
        }
    }
    // move b next to the a_c so one multi-value reduction covers all Cn+1 sums
    float vals[MC + 1];
#pragma unroll
    for (int c = 0; c < MC; ++c) vals[c] = acc[c];
    vals[MC] = 0.f;
#pragma unroll
    for (int c = 0; c <= MC; ++c) if (c == d.Cn) vals[c] = acc[MC];
    block_sum_multi<MC>(vals, d.Cn + 1, part, red, t, live);
    if (live && t <= d.Cn) b.p[SP_TMP][d.part_off + blk * (COMBINE_MAXC + 1) + t] = red[t];
}

// g, x and (when the site accumulates) the old gx of U trips, all in flight together
template <int MC, int U, bool FIRST>
__device__ __forceinline__ void combine_load_bwd(const CombineDesc& d, comb_gptr x, comb_gptr go, comb_gptr gx, const unsigned e0, const unsigned stride,
                                                 const unsigned n, float (&v)[U][MC], float (&old)[U][MC], float (&g)[U], int64_t (&eo)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned e = e0 + u * stride;
        g[u] = go[e < n ? e : 0u];
    }
    combine_load_x<MC, U>(d, x, e0, stride, n, v, eo);
    if (!FIRST) combine_load_x<MC, U>(d, gx, e0, stride, n, old, eo);
}

// dx_c = g fa_c + fb_c x_c with the per-channel factors fa_c = n_c / S, fb_c = ((a_c - b) / S) / n_c; FIRST: the site is the
// first writer of gx in this pass and stores instead of adding (workgroup-uniform: decided once, outside the loops)
template <int MC, bool FIRST>
__device__ __forceinline__ void combine_bwd_apply_body(const CombineDesc& d, const int blk, const int t, const Bases& b,
                                                       float* coef, float* nc_s, float (*part)[COMBINE_MAXC + 1]) {
    constexpr int U = CombineTrips<MC>::U;
    float* gr = b.p[SP_GRAD];
    comb_gptr tmp = (comb_gptr)b.p[SP_TMP];
    comb_gptr x = (comb_gptr)b.p[SP_WS] + d.x_off;
    comb_gptr go = (comb_gptr)gr + d.gout_off;
    comb_gptr gx = (comb_gptr)gr + d.gx_off;
    const unsigned n = (unsigned)(d.rows * d.cols), stride = (unsigned)d.nblk * 256u;
    unsigned e0 = (unsigned)blk * 256u + t;
    float v[U][MC], old[U][MC], g[U];
    int64_t eo[U];
    {   // partials, stats and the first group of trips are all loaded in front of the reduction
        float vals[MC + 1];
        combine_load_bwd<MC, U, FIRST>(d, x, go, gx, e0, stride, n, v, old, g, eo);
        combine_load_partials<MC>(d, tmp, t, d.Cn + 1, vals);
        const float st = tmp[d.stats_off + (t <= d.Cn ? t : 0)];       // n_c ..., S
        MST_SCHED_FENCE();       // (the scheduler otherwise starts the reduction, and waits, in front of the x loads)
        if (t <= d.Cn) nc_s[t] = st;
        block_sum_multi<MC>(vals, d.Cn + 1, part, coef, t);
    }
    const float S = nc_s[d.Cn];
    const float bsum = coef[d.Cn];
    float fa[MC], fb[MC];
#pragma unroll
    for (int c = 0; c < MC; ++c) {
        const float nc = c < d.Cn ? nc_s[c] : 1.f;
        fa[c] = nc / S; fb[c] = c < d.Cn ? ((coef[c] - bsum) / S) / nc : 0.f;
    }
    while (e0 < n) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (e0 + u * stride < n) {
#pragma unroll
                for (int c = 0; c < MC; ++c) {
                    if (c < d.Cn) {
                        const float w = fmaf(g[u], fa[c], fb[c] * v[u][c]);
                        gr[d.gx_off + (int64_t)c * d.cs + eo[u]] = FIRST ? w : old[u][c] + w;
                    }
                }
            }
        }
        e0 += stride * U;
        if (e0 < n) combine_load_bwd<MC, U, FIRST>(d, x, go, gx, e0, stride, n, v, old, g, eo);
    }
}

// Small sites (<= COMBINE_SMALL elements per slice: the per-bar tensors, the style vector) need no cross-workgroup
// re-sum: one 256-lane group per site does reduction and elementwise pass.  One group walks the whole site, and a trip per
// element was a chain of n / 256 dependent L2 round trips (16 us for 4096 elements): U elements per lane and trip.
template <int MC>
__device__ __forceinline__ void combine_small_fwd_body(const CombineDesc& d, const int t, const bool live, const Bases& b,
                                                       float (*part)[COMBINE_MAXC + 1], float* red) {
    constexpr int U = CombineTrips<MC>::U;
    float* ws = b.p[SP_WS];
    float* tmp = b.p[SP_TMP];
    comb_gptr x = (comb_gptr)ws + d.x_off;
    const unsigned n = live ? (unsigned)(d.rows * d.cols) : 0u;
    float acc[MC + 1];
#pragma unroll
    for (int c = 0; c <= MC; ++c) acc[c] = 0.f;
    for (unsigned e0 = t; e0 < n; e0 += 256 * U) {
        float v[U][MC];
        int64_t eo[U];
        combine_load_x<MC, U>(d, x, e0, 256u, n, v, eo);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool ok = e0 + 256 * u < n;
#pragma unroll
            for (int c = 0; c < MC; ++c) acc[c] = (ok && c < d.Cn) ? fmaf(v[u][c], v[u][c], acc[c]) : acc[c];
        }
    }
    block_sum_multi<MC>(acc, d.Cn, part, red, t, live);
    float nc[MC], S;
    combine_norms<MC>(d, red, nc, S);
    if (live && t <= d.Cn) tmp[d.stats_off + t] = t < d.Cn ? sqrtf(1.f + red[t]) : S;
    for (unsigned e0 = t; e0 < n; e0 += 256 * U) {
        float v[U][MC];
        int64_t eo[U];
        combine_load_x<MC, U>(d, x, e0, 256u, n, v, eo);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned e = e0 + 256 * u;
            float a = 0.f;
#pragma unroll
            for (int c = 0; c < MC; ++c) if (c < d.Cn) a += v[u][c] * nc[c];
            if (e < n) ws[d.out_off + e] = a / S;
        }
    }
}

template <int MC, bool FIRST>
__device__ __forceinline__ void combine_small_bwd_body(const CombineDesc& d, const int t, const bool live, const Bases& b,
                                                       float* coef, float* nc_s, float (*part)[COMBINE_MAXC + 1]) {
    constexpr int U = CombineTrips<MC>::U;
    float* gr = b.p[SP_GRAD];
    comb_gptr tmp = (comb_gptr)b.p[SP_TMP];
    comb_gptr x = (comb_gptr)b.p[SP_WS] + d.x_off;
    comb_gptr out = (comb_gptr)b.p[SP_WS] + d.out_off;
    comb_gptr go = (comb_gptr)gr + d.gout_off;
    comb_gptr gx = (comb_gptr)gr + d.gx_off;
    const unsigned n = live ? (unsigned)(d.rows * d.cols) : 0u;
    const float st = live ? tmp[d.stats_off + (t <= d.Cn ? t : 0)] : 0.f;       // n_c ..., S: loaded in front of the reduction
    float acc[MC + 1];
#pragma unroll
    for (int c = 0; c <= MC; ++c) acc[c] = 0.f;
    for (unsigned e0 = t; e0 < n; e0 += 256 * U) {
        float v[U][MC], g[U], o[U];
        int64_t eo[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned e = e0 + 256 * u, ec = e < n ? e : 0u;
            g[u] = go[ec];
            o[u] = out[ec];
        }
        combine_load_x<MC, U>(d, x, e0, 256u, n, v, eo);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool ok = e0 + 256 * u < n;
#pragma unroll
            for (int c = 0; c < MC; ++c) acc[c] = (ok && c < d.Cn) ? fmaf(g[u], v[u][c], acc[c]) : acc[c];
            acc[MC] = ok ? fmaf(g[u], o[u], acc[MC]) : acc[MC];
        }
    }
    float vals[MC + 1];
#pragma unroll
    for (int c = 0; c < MC; ++c) vals[c] = acc[c];
    vals[MC] = 0.f;
#pragma unroll
    for (int c = 0; c <= MC; ++c) if (c == d.Cn) vals[c] = acc[MC];
    if (live && t <= d.Cn) nc_s[t] = st;
    block_sum_multi<MC>(vals, d.Cn + 1, part, coef, t, live);
    const float S = nc_s[d.Cn];
    const float bsum = coef[d.Cn];
    // per-channel factors once per lane (two IEEE divisions per element and channel were most of the elementwise pass):
    // dx_c = g n_c / S + ((b_c - b) / S) x_c / n_c
    float fa[MC], fb[MC];
#pragma unroll
    for (int c = 0; c < MC; ++c) {
        const float nc = c < d.Cn ? nc_s[c] : 1.f;
        fa[c] = nc / S; fb[c] = c < d.Cn ? ((coef[c] - bsum) / S) / nc : 0.f;
    }
    for (unsigned e0 = t; e0 < n; e0 += 256 * U) {
        float v[U][MC], old[U][MC], g[U];
        int64_t eo[U];
        combine_load_bwd<MC, U, FIRST>(d, x, go, gx, e0, 256u, n, v, old, g, eo);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (e0 + 256 * u < n) {
#pragma unroll
                for (int c = 0; c < MC; ++c) {
                    if (c < d.Cn) {
                        const float w = fmaf(g[u], fa[c], fb[c] * v[u][c]);
                        gr[d.gx_off + (int64_t)c * d.cs + eo[u]] = FIRST ? w : old[u][c] + w;
                    }
                }
            }
        }
    }
}
