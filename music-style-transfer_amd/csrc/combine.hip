// combine() of style/model.py:796-815 for gfx950: a norm-weighted merge over the channel axis,
//   n_c = sqrt(1 + sum(x_c^2)),  out = sum_c x_c n_c / sum_c n_c,
// and its exact backward (the gradient flows through the norms as well):
//   dx_c = g n_c / S + ((a_c - b) / S) x_c / n_c,  a_c = sum(g x_c),  b = sum(g out),  S = sum_c n_c.
// Both directions are a global reduction followed by an elementwise pass, so each is two
// launches; partial sums are written per workgroup and re-summed in index order by every
// consumer workgroup (deterministic, no float atomics).  blockIdx.y selects the call site, so
// independent sites of one dependency level share launches.  HBM/L2-bound: x is read twice per
// direction, coalesced along the feature axis; the backward reduce reads g once for all channels.
#include "combine_body.h"

// The bodies are in combine_body.h (gemm_kernel runs them too, for the combine steps its launch carries); the kernels here are
// the stand-alone launches: blockIdx.x = the site's workgroup, blockIdx.y = the site.
// MC: compile-time bound on the channel count (4: every site of the model up to 4 channels — unrolled loops and shuffle
// reductions over 32 mostly absent channels were most of the small kernels' ~10 us; 32: the general case)
// whole_small: a site of at most COMBINE_SMALL elements per slice that shares the two-launch step with larger ones runs its whole
// step in workgroup 0 of the first launch, on the body the one-launch kernels run (the same sums in the same order, and no partial
// sums left in scratch, whatever else the site's level holds); 0 for the halves of a tiled plan, whose partial sums meet the
// other ranks' between the launches
template <int MC>
__global__ __launch_bounds__(256) void combine_sumsq_kernel(const CombineDesc* __restrict__ descs, Bases b, int whole_small) {
    const CombineDesc d = descs[blockIdx.y];     // by value: fields stay in registers across barriers
    if ((int)blockIdx.x >= d.nblk) return;
    __shared__ float part[4][COMBINE_MAXC + 1];
    __shared__ float red[COMBINE_MAXC + 1];
    if (whole_small && combine_site_small(d)) {
        if (blockIdx.x == 0) combine_small_fwd_body<MC>(d, threadIdx.x, true, b, part, red);
        return;
    }
    combine_sumsq_body<MC>(d, blockIdx.x, threadIdx.x, true, b, part, red);
}

template <int MC>
__global__ __launch_bounds__(256) void combine_apply_kernel(const CombineDesc* __restrict__ descs, Bases b, int whole_small) {
    const CombineDesc d = descs[blockIdx.y];
    if ((int)blockIdx.x >= d.nblk || (whole_small && combine_site_small(d))) return;
    __shared__ float part[4][COMBINE_MAXC + 1];
    __shared__ float red[COMBINE_MAXC + 1];
    combine_apply_body<MC>(d, blockIdx.x, threadIdx.x, b, part, red);
}

template <int MC>
__global__ __launch_bounds__(256) void combine_bwd_reduce_kernel(const CombineDesc* __restrict__ descs, Bases b, int whole_small) {
    const CombineDesc d = descs[blockIdx.y];
    if ((int)blockIdx.x >= d.nblk) return;
    __shared__ float nc_s[COMBINE_MAXC + 1];
    __shared__ float part[4][COMBINE_MAXC + 1];
    __shared__ float red[COMBINE_MAXC + 1];
    if (whole_small && combine_site_small(d)) {
        if (blockIdx.x == 0) {
            if (d.first) combine_small_bwd_body<MC, true>(d, threadIdx.x, true, b, red, nc_s, part);
            else combine_small_bwd_body<MC, false>(d, threadIdx.x, true, b, red, nc_s, part);
        }
        return;
    }
    combine_bwd_reduce_body<MC>(d, blockIdx.x, threadIdx.x, true, b, part, red);
}

template <int MC>
__global__ __launch_bounds__(256) void combine_bwd_apply_kernel(const CombineDesc* __restrict__ descs, Bases b, int whole_small) {
    const CombineDesc d = descs[blockIdx.y];
    if ((int)blockIdx.x >= d.nblk || (whole_small && combine_site_small(d))) return;
    __shared__ float coef[COMBINE_MAXC + 1];
    __shared__ float nc_s[COMBINE_MAXC + 1];
    __shared__ float part[4][COMBINE_MAXC + 1];
    if (d.first) combine_bwd_apply_body<MC, true>(d, blockIdx.x, threadIdx.x, b, coef, nc_s, part);
    else combine_bwd_apply_body<MC, false>(d, blockIdx.x, threadIdx.x, b, coef, nc_s, part);
}

template <int MC>
__global__ __launch_bounds__(256) void combine_small_fwd_kernel(const CombineDesc* __restrict__ descs, Bases b) {
    const CombineDesc d = descs[blockIdx.x];
    __shared__ float part[4][COMBINE_MAXC + 1];
    __shared__ float red[COMBINE_MAXC + 1];
    combine_small_fwd_body<MC>(d, threadIdx.x, true, b, part, red);
}

template <int MC>
__global__ __launch_bounds__(256) void combine_small_bwd_kernel(const CombineDesc* __restrict__ descs, Bases b) {
    const CombineDesc d = descs[blockIdx.x];
    __shared__ float coef[COMBINE_MAXC + 1];
    __shared__ float nc_s[COMBINE_MAXC + 1];
    __shared__ float part[4][COMBINE_MAXC + 1];
    if (d.first) combine_small_bwd_body<MC, true>(d, threadIdx.x, true, b, coef, nc_s, part);
    else combine_small_bwd_body<MC, false>(d, threadIdx.x, true, b, coef, nc_s, part);
}

// all_small: every site of the (merged) launch has <= COMBINE_SMALL elements per slice (2: and at most 4 channels)
// mc4: no site of the plan has more than 4 channels (the large kernels' MC = 4 flavour)
int launch_combine_fwd(const CombineDesc* dev, int count, int max_nblk, int all_small, int mc4, Bases b, hipStream_t s) {
    if (count <= 0) return 0;
    if (all_small) {
        if (all_small == 2) hipLaunchKernelGGL(combine_small_fwd_kernel<4>, dim3(count), dim3(256), 0, s, dev, b);
        else hipLaunchKernelGGL(combine_small_fwd_kernel<COMBINE_MAXC>, dim3(count), dim3(256), 0, s, dev, b);
        return (int)hipGetLastError();
    }
    if (int e = launch_combine_phase(dev, max_nblk, 0, b, s, count, mc4, 1)) return e;
    return launch_combine_phase(dev, max_nblk, 1, b, s, count, mc4, 1);
}

int launch_combine_bwd(const CombineDesc* dev, int count, int max_nblk, int all_small, int mc4, Bases b, hipStream_t s) {
    if (count <= 0) return 0;
    if (all_small) {
        if (all_small == 2) hipLaunchKernelGGL(combine_small_bwd_kernel<4>, dim3(count), dim3(256), 0, s, dev, b);
        else hipLaunchKernelGGL(combine_small_bwd_kernel<COMBINE_MAXC>, dim3(count), dim3(256), 0, s, dev, b);
        return (int)hipGetLastError();
    }
    if (int e = launch_combine_phase(dev, max_nblk, 2, b, s, count, mc4, 1)) return e;
    return launch_combine_phase(dev, max_nblk, 3, b, s, count, mc4, 1);
}

// ---- tiled plans: the halves of a combine on their own (the ranks' partial sums meet in between), strided row copies
// and the fold / spread pair around an exchange (mst_common.h)
int launch_combine_phase(const CombineDesc* dev, int nblk, int which, Bases b, hipStream_t s, int count, int mc4, int whole_small) {
    const dim3 grid(nblk, count), lanes(256);
#define COMBINE_PHASE(K) do { if (mc4) hipLaunchKernelGGL(K<4>, grid, lanes, 0, s, dev, b, whole_small); else hipLaunchKernelGGL(K<COMBINE_MAXC>, grid, lanes, 0, s, dev, b, whole_small); } while (0)
    if (which == 0) COMBINE_PHASE(combine_sumsq_kernel);
    else if (which == 1) COMBINE_PHASE(combine_apply_kernel);
    else if (which == 2) COMBINE_PHASE(combine_bwd_reduce_kernel);
    else COMBINE_PHASE(combine_bwd_apply_kernel);
#undef COMBINE_PHASE
    return (int)hipGetLastError();
}

__global__ __launch_bounds__(256) void copy_rows_kernel(const CopyDesc* __restrict__ dp, int backward, Bases b) {
    const CopyDesc d = dp[0];
    const int total = d.na * d.nb * d.cols;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
        const int j = e % d.cols, ab = e / d.cols, bb = ab % d.nb, a = ab / d.nb;
        const int64_t so = d.src_off + (int64_t)a * d.src_sa + (int64_t)bb * d.src_sb + j;
        const int64_t dof = d.dst_off + (int64_t)a * d.dst_sa + (int64_t)bb * d.dst_sb + j;
        if (!backward) b.p[SP_WS][dof] = b.p[SP_WS][so];
        else { float* g = b.p[SP_GRAD] + so; const float v = b.p[SP_GRAD][dof]; *g = d.first ? v : *g + v; }
    }
}

int launch_copy_rows(const CopyDesc* dev, const CopyDesc& host, int backward, Bases b, hipStream_t s) {
    const int total = host.na * host.nb * host.cols;
    int nb = (total + 255) / 256;
    if (nb > 1024) nb = 1024;
    if (nb < 1) return 0;
    hipLaunchKernelGGL(copy_rows_kernel, dim3(nb), dim3(256), 0, s, dev, backward, b);
    return (int)hipGetLastError();
}

__global__ __launch_bounds__(64) void fold_kernel(const FoldDesc* __restrict__ dp, int spread, Bases b) {
    const FoldDesc d = dp[0];
    float* part = b.p[d.space] + d.part_off;
    float* sum = b.p[SP_TMP] + d.sum_off;
    for (int c = threadIdx.x; c < d.ncols; c += 64) {
        if (!spread) {
            float a = 0.f;
            for (int r = 0; r < d.nrows; ++r) a += part[(int64_t)r * d.row_stride + (int64_t)c * d.col_stride];
            sum[c] = a;
        } else {
            part[(int64_t)c * d.col_stride] = sum[c];
            for (int r = 1; r < d.nrows; ++r) part[(int64_t)r * d.row_stride + (int64_t)c * d.col_stride] = 0.f;
        }
    }
}

int launch_fold(const FoldDesc* dev, int spread, Bases b, hipStream_t s) {
    hipLaunchKernelGGL(fold_kernel, dim3(1), dim3(64), 0, s, dev, spread, b);
    return (int)hipGetLastError();
}
