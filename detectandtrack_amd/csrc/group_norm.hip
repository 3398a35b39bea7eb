// GroupNorm (HIP.USE_GN) on NDHWC blobs [clips][rows][cstride]: per-clip group statistics, normalise (+ residual, ReLU), and the two
// backward passes.  DESIGN.md section 3.11.  The heavy kernels (statistics partials, apply, backward reduce: norm_kernels.h) are the
// ones of SpatialBN with a clip dimension in the grid; they work per (clip, channel) and know nothing about groups.  Groups exist in
// two tiny kernels only, one per direction: they fold the per-channel results of a clip into its G groups -- any cg = C / G, also one
// that is no power of two or whose groups straddle the 64-channel chunks of the thread layout -- and write per-(clip, channel) tables,
// so that the passes over the blob are one fma per element again.
//
// Determinism and independence: every merge runs in a fixed order that depends on the clip's own shape only, and no block reads
// another clip's rows, partials or tables -- a clip gets the same bits alone and among others.  No float atomics.
#include "norm_kernels.h"

namespace {

// ---- forward: (clip, channel) = the merge of that channel's block partials ------------------------------------------------------------
// grid (chunks, clips), GN_ML lanes per channel: lane l merges the partial rows l, l + GN_ML, ... in order, lane 0 then merges the lanes
// in order.  (One 64-channel chunk may hold ~1000 partial rows: a chain of 64 + 16 dependent merges, not of 256 + 4, and without a
// branch in the loop, so that the loads of the next rows are in flight while a row is merged.  A block that saw no row has count 0:
// its weight f is 0 and it changes nothing.)
constexpr int GN_ML = 16, GN_MERGE_BLOCK = 64 * GN_ML;

__device__ __forceinline__ void chan_merge(float& n, float& mean, float& m2, float nb, float mb, float qb) {
    const float nn = n + nb, f = nn > 0.f ? nb / nn : 0.f, d = mb - mean;
    mean += d * f;
    m2 += qb + d * d * (n * f);
    n = nn;
}

__global__ void __launch_bounds__(GN_MERGE_BLOCK) gn_channel_merge_kernel(const float* __restrict__ pmean, const float* __restrict__ pm2,
                                                                          const float* __restrict__ pcnt, int nblk, int cs,
                                                                          float* __restrict__ cmean, float* __restrict__ cm2) {
    const int cl = threadIdx.x & 63, lane = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const size_t clip = blockIdx.y;
    pmean += clip * nblk * cs;
    pm2 += clip * nblk * cs;
    pcnt += (clip * gridDim.x + blockIdx.x) * nblk;
    float n = 0.f, mean = 0.f, m2 = 0.f;
#pragma unroll 4
    for (int b = lane; b < nblk; b += GN_ML) chan_merge(n, mean, m2, pcnt[b], pmean[(size_t)b * cs + c], pm2[(size_t)b * cs + c]);
    __shared__ float s[3][GN_MERGE_BLOCK];
    s[0][threadIdx.x] = n; s[1][threadIdx.x] = mean; s[2][threadIdx.x] = m2;
    __syncthreads();
    if (lane != 0) return;
    for (int j = 1; j < GN_ML; ++j) chan_merge(n, mean, m2, s[0][j * 64 + cl], s[1][j * 64 + cl], s[2][j * 64 + cl]);
    cmean[clip * cs + c] = mean;
    cm2[clip * cs + c] = m2;
}

// grid (clips): a thread per group merges the group's cg channels (each over `rows` positions) in channel order with Chan's formula and
// writes the tables of its channels: mean, rstd (equal within the group), a = scale * rstd, b' = bias - mean * a.  The threads then
// zero the padding channels.  The padding channels of cmean / cm2 (whatever the blob's padding held) are never read.
// cmean[c] is the mean of z - shift[c] (bn_stats_partial_kernel): the group works relative to the shift of its first channel, Kg, with
// channel c's mean moved by shift[c] - Kg (two data values: exact, or rounded relative to a difference that is then real spread), and
// adds Kg to the merged mean at the very end.
__global__ void __launch_bounds__(BN_BLOCK) gn_stats_finalize_kernel(const float* __restrict__ cmean, const float* __restrict__ cm2,
                                                                     const float* __restrict__ shift, long long rows, int cs, int C, int G,
                                                                     const float* __restrict__ scale, const float* __restrict__ bias,
                                                                     float eps, float* __restrict__ mean_out,
                                                                     float* __restrict__ rstd_out, float* __restrict__ a_out,
                                                                     float* __restrict__ b_out) {
    const size_t at = (size_t)blockIdx.x * cs;
    const int cg = C / G;
    const float nb = (float)rows;
    for (int g = threadIdx.x; g < G; g += BN_BLOCK) {
        const int c0 = g * cg;
        const float Kg = shift[at + c0];
        float n = nb, mean = cmean[at + c0], m2 = cm2[at + c0];
        for (int c = c0 + 1; c < c0 + cg; ++c) {
            const float nn = n + nb, f = nb / nn, d = (cmean[at + c] + (shift[at + c] - Kg)) - mean;
            mean += d * f;
            m2 += cm2[at + c] + d * d * (n * f);
            n = nn;
        }
        mean += Kg;
        const float var = m2 / (nb * (float)cg);
        const float rstd = 1.f / sqrtf(var + eps);
        for (int c = c0; c < c0 + cg; ++c) {
            const float a = scale[c] * rstd;
            mean_out[at + c] = mean;
            rstd_out[at + c] = rstd;
            a_out[at + c] = a;
            b_out[at + c] = bias[c] - mean * a;
        }
    }
    for (int c = C + threadIdx.x; c < cs; c += BN_BLOCK) mean_out[at + c] = rstd_out[at + c] = a_out[at + c] = b_out[at + c] = 0.f;
}

// ---- backward: sums[clip][0][c] = sum g, sums[clip][1][c] = sum g * xhat of the clip's window; dbeta / dgamma += the sum over the clips ----
// grid (chunks): the clips in order; GN_ML lanes per channel sum every GN_ML-th partial row in order, lane 0 sums the lanes in order
__global__ void __launch_bounds__(GN_MERGE_BLOCK) gn_bwd_finalize_kernel(const float* __restrict__ pdb, const float* __restrict__ pds,
                                                                         int nblk, int clips, int cs, int C, float* __restrict__ sums,
                                                                         float* __restrict__ dbeta, float* __restrict__ dgamma) {
    const int cl = threadIdx.x & 63, lane = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    __shared__ float sh[2][GN_MERGE_BLOCK];
    float tb = 0.f, ts = 0.f;
    for (int n = 0; n < clips; ++n) {
        const float* qb = pdb + (size_t)n * nblk * cs;
        const float* qs = pds + (size_t)n * nblk * cs;
        float b = 0.f, s = 0.f;
#pragma unroll 4
        for (int k = lane; k < nblk; k += GN_ML) {
            b += qb[(size_t)k * cs + c];
            s += qs[(size_t)k * cs + c];
        }
        __syncthreads();
        sh[0][threadIdx.x] = b; sh[1][threadIdx.x] = s;
        __syncthreads();
        if (lane == 0) {
            for (int j = 1; j < GN_ML; ++j) {
                b += sh[0][j * 64 + cl];
                s += sh[1][j * 64 + cl];
            }
            if (c >= C) b = s = 0.f;
            sums[((size_t)n * 2) * cs + c] = b;
            sums[((size_t)n * 2 + 1) * cs + c] = s;
            tb += b;
            ts += s;
        }
    }
    if (lane == 0 && c < C) {
        if (dbeta) dbeta[c] += tb;
        if (dgamma) dgamma[c] += ts;
    }
}

// grid (clips): a thread per group sums A = sum_c scale[c] S1[c], B = sum_c scale[c] S2[c] over the group's channels in order and writes
// the coefficients of  dz = a g + q + r (z - mean):  q = -rstd A / Mg,  r = -rstd^2 B / Mg,  Mg = rows * cg  (zeros in the padding)
__global__ void __launch_bounds__(BN_BLOCK) gn_bwd_coef_kernel(const float* __restrict__ sums, const float* __restrict__ rstd,
                                                               const float* __restrict__ scale, long long rows, int cs, int C, int G,
                                                               float* __restrict__ coef) {
    const size_t n = blockIdx.x;
    const float* s1 = sums + n * 2 * cs;
    const float* s2 = s1 + cs;
    float* q = coef + n * 2 * cs;
    float* r = q + cs;
    const int cg = C / G;
    const float invMg = 1.f / ((float)rows * (float)cg);
    for (int g = threadIdx.x; g < G; g += BN_BLOCK) {
        const int c0 = g * cg;
        float A = 0.f, B = 0.f;
        for (int c = c0; c < c0 + cg; ++c) {
            A = fmaf(scale[c], s1[c], A);
            B = fmaf(scale[c], s2[c], B);
        }
        const float rs = rstd[n * cs + c0];
        const float qv = -(rs * A) * invMg, rv = -(rs * rs * B) * invMg;
        for (int c = c0; c < c0 + cg; ++c) {
            q[c] = qv;
            r[c] = rv;
        }
    }
    for (int c = C + threadIdx.x; c < cs; c += BN_BLOCK) q[c] = r[c] = 0.f;
}

// ---- backward: dz = a g + q + r (z - mean) on EVERY row of every clip (g = 0 outside [row_lo, row_lo + nrows)) ---------------------------
// (z - mean, not r z + (q - r mean): the difference is the small number, also for a clip whose mean is far from zero)
template <int DT>
__global__ void __launch_bounds__(BN_BLOCK) gn_bwd_apply_kernel(const void* __restrict__ g, const void* __restrict__ z, void* __restrict__ dz,
                                                                const float* __restrict__ mean, const float* __restrict__ a,
                                                                const float* __restrict__ coef, long long rows, long long row_lo,
                                                                long long nrows, int C, int cs) {
    typedef Lane<DT> L;
    constexpr int VEC = L::VEC;
    const L ln;
    const size_t zbase = ln.clip * (size_t)rows * cs, gbase = ln.clip * (size_t)nrows * cs;
    float mu[VEC], ka[VEC], kq[VEC], kr[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        mu[e] = mean[ln.clip * cs + ln.c0 + e];
        ka[e] = a[ln.clip * cs + ln.c0 + e];
        kq[e] = coef[ln.clip * 2 * cs + ln.c0 + e];
        kr[e] = coef[(ln.clip * 2 + 1) * cs + ln.c0 + e];
    }
    for (long long r = ln.row0; r < rows; r += ln.step * BN_U) {
        float x[BN_U][VEC], gv[BN_U][VEC];
#pragma unroll
        for (int u = 0; u < BN_U; ++u) {
            const long long rr = r + ln.step * u;
            const long long rc = rr < rows ? rr : r;
            Vec<DT>::ld(z, zbase + (size_t)rc * cs + ln.c0, x[u]);
            const long long w = rc - row_lo;
            if (w >= 0 && w < nrows) {
                Vec<DT>::ld(g, gbase + (size_t)w * cs + ln.c0, gv[u]);
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e) gv[u][e] = 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < BN_U; ++u) {
            const long long rr = r + ln.step * u;
            if (rr >= rows) break;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float o = fmaf(ka[e], gv[u][e], fmaf(kr[e], x[u][e] - mu[e], kq[e]));
                x[u][e] = ln.c0 + e < C ? o : 0.f;
            }
            Vec<DT>::st(dz, zbase + (size_t)rr * cs + ln.c0, x[u]);
        }
    }
}

// floats of the workspace for `clips` clips of `rows` rows: the statistics partials (mean, M2: [clips][blocks][cs]; counts:
// [clips][chunks][blocks]), the per-channel merge ([clips][cs] mean, M2) and the shift ([clips][cs]).  The backward partials of a window (two
// [clips][blocks][cs], blocks of at most as many rows) fit into the same bytes.
size_t gn_ws_floats(int dtype, int clips, long long rows, int cs) {
    const size_t nblk = bn_row_blocks(dtype, rows, cs);
    return (size_t)clips * (nblk * (2 * (size_t)cs + cs / 64) + 3 * (size_t)cs);
}

}  // namespace

size_t dat_gn_workspace_bytes(int dtype, int clips, long long rows, int cstride) {
    if (clips < 1 || clips > 65535 || rows < 1 || cstride < 64 || cstride % 64 != 0) return 0;
    return gn_ws_floats(dtype, clips, rows, cstride) * sizeof(float);
}

static int gn_check_shape(dat_ctx* ctx, const char* what, int dtype, int clips, long long rows, int C, int cs) {
    DAT_ENFORCE(ctx, dtype == DAT_F32 || dtype == DAT_BF16, "%s: dtype %d", what, dtype);
    DAT_ENFORCE(ctx, clips >= 1 && clips <= 65535, "%s: %d clips", what, clips);
    DAT_ENFORCE(ctx, rows >= 1 && rows * (long long)cs < (1ll << 40) / clips, "%s: %d clips of %lld rows", what, clips, rows);
    DAT_ENFORCE(ctx, cs >= 64 && cs % 64 == 0 && C >= 1 && C <= cs, "%s: %d channels at stride %d (a multiple of 64)", what, C, cs);
    return DAT_OK;
}

static int gn_check_groups(dat_ctx* ctx, const char* what, long long rows, int C, int groups) {
    DAT_ENFORCE(ctx, groups >= 1 && C % groups == 0, "%s: %d channels in %d groups", what, C, groups);
    DAT_ENFORCE(ctx, rows * (C / groups) >= 2, "%s: group statistics need at least 2 values per group (got %lld)", what,
                rows * (C / groups));
    return DAT_OK;
}

// the backward call shapes the executor produces: every frame of N >= 1 clips, or a frame window of ONE clip
static int gn_check_window(dat_ctx* ctx, const char* what, int clips, long long rows, long long row_lo, long long nrows) {
    DAT_ENFORCE(ctx, row_lo >= 0 && nrows >= 1 && row_lo + nrows <= rows, "%s: window [%lld, %lld) of %lld rows", what, row_lo,
                row_lo + nrows, rows);
    DAT_ENFORCE(ctx, clips == 1 || (row_lo == 0 && nrows == rows), "%s: a frame window [%lld, %lld) of %lld rows with %d clips (one clip only)",
                what, row_lo, row_lo + nrows, rows, clips);
    return DAT_OK;
}

int dat_gn_stats(dat_ctx* ctx, dat_stream s, int dtype, const void* z, int clips, long long rows, int C, int cstride, int groups,
                 const float* scale, const float* bias, float eps, float* mean, float* rstd, float* a, float* bprime, void* ws,
                 size_t ws_bytes) {
    int rc = gn_check_shape(ctx, "gn_stats", dtype, clips, rows, C, cstride);
    if (rc != DAT_OK) return rc;
    rc = gn_check_groups(ctx, "gn_stats", rows, C, groups);
    if (rc != DAT_OK) return rc;
    DAT_ENFORCE(ctx, z && scale && bias && mean && rstd && a && bprime && ws, "gn_stats: null argument");
    DAT_ENFORCE(ctx, aligned16(z), "gn_stats: z must be 16-byte aligned");
    const size_t need = gn_ws_floats(dtype, clips, rows, cstride) * sizeof(float);
    DAT_ENFORCE(ctx, ws_bytes >= need, "gn_stats: workspace of %zu bytes, %zu needed", ws_bytes, need);
    const int nblk = bn_row_blocks(dtype, rows, cstride), chunks = cstride / 64;
    float* pmean = (float*)ws;
    float* pm2 = pmean + (size_t)clips * nblk * cstride;
    float* pcnt = pm2 + (size_t)clips * nblk * cstride;
    float* cmean = pcnt + (size_t)clips * chunks * nblk;
    float* cm2 = cmean + (size_t)clips * cstride;
    float* shift = cm2 + (size_t)clips * cstride;
    BN_LAUNCH(bn_stats_partial_kernel, dim3(nblk, chunks, clips), s, z, rows, cstride, pmean, pm2, pcnt, shift);
    hipLaunchKernelGGL(gn_channel_merge_kernel, dim3(chunks, clips), dim3(GN_MERGE_BLOCK), 0, (hipStream_t)s, (const float*)pmean,
                       (const float*)pm2, (const float*)pcnt, nblk, cstride, cmean, cm2);
    hipLaunchKernelGGL(gn_stats_finalize_kernel, dim3(clips), dim3(BN_BLOCK), 0, (hipStream_t)s, (const float*)cmean, (const float*)cm2,
                       (const float*)shift, rows, cstride, C, groups, scale, bias, eps, mean, rstd, a, bprime);
    DAT_CHECK_LAUNCH(ctx, "gn_stats");
    return DAT_OK;
}

int dat_gn_apply(dat_ctx* ctx, dat_stream s, int dtype, const void* z, const void* residual, void* y, const float* a, const float* bprime,
                 int clips, long long rows, int C, int cstride, int relu) {
    int rc = gn_check_shape(ctx, "gn_apply", dtype, clips, rows, C, cstride);
    if (rc != DAT_OK) return rc;
    DAT_ENFORCE(ctx, z && y && a && bprime, "gn_apply: null argument");
    DAT_ENFORCE(ctx, aligned16(z) && aligned16(y) && aligned16(residual), "gn_apply: tensors must be 16-byte aligned");
    BN_LAUNCH(bn_apply_kernel, dim3(bn_row_blocks(dtype, rows, cstride), cstride / 64, clips), s, z, residual, y, a, bprime, rows, C,
              cstride, relu);
    DAT_CHECK_LAUNCH(ctx, "gn_apply");
    return DAT_OK;
}

int dat_gn_bwd_reduce(dat_ctx* ctx, dat_stream s, int dtype, const void* dy, const void* y, const void* z, void* g, const float* mean,
                      const float* rstd, const float* scale, int clips, long long rows, long long row_lo, long long nrows, int C,
                      int cstride, int groups, int relu, float* sums, float* coef, float* dbeta, float* dgamma, void* ws, size_t ws_bytes) {
    int rc = gn_check_shape(ctx, "gn_bwd_reduce", dtype, clips, rows, C, cstride);
    if (rc != DAT_OK) return rc;
    rc = gn_check_groups(ctx, "gn_bwd_reduce", rows, C, groups);
    if (rc != DAT_OK) return rc;
    rc = gn_check_window(ctx, "gn_bwd_reduce", clips, rows, row_lo, nrows);
    if (rc != DAT_OK) return rc;
    DAT_ENFORCE(ctx, dy && z && g && mean && rstd && scale && sums && coef && ws && (y || !relu), "gn_bwd_reduce: null argument");
    DAT_ENFORCE(ctx, aligned16(dy) && aligned16(y) && aligned16(z) && aligned16(g), "gn_bwd_reduce: tensors must be 16-byte aligned");
    const int nblk = bn_row_blocks(dtype, nrows, cstride), chunks = cstride / 64;
    const size_t need = (size_t)clips * nblk * 2 * cstride * sizeof(float);
    DAT_ENFORCE(ctx, ws_bytes >= need, "gn_bwd_reduce: workspace of %zu bytes, %zu needed", ws_bytes, need);
    float* pdb = (float*)ws;
    float* pds = pdb + (size_t)clips * nblk * cstride;
    BN_LAUNCH(bn_bwd_reduce_kernel, dim3(nblk, chunks, clips), s, dy, y, z, g, mean, rstd, rows, row_lo, nrows, C, cstride, relu, pdb, pds);
    hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3(chunks), dim3(GN_MERGE_BLOCK), 0, (hipStream_t)s, (const float*)pdb, (const float*)pds, nblk,
                       clips, cstride, C, sums, dbeta, dgamma);
    hipLaunchKernelGGL(gn_bwd_coef_kernel, dim3(clips), dim3(BN_BLOCK), 0, (hipStream_t)s, (const float*)sums, rstd, scale, rows, cstride, C,
                       groups, coef);
    DAT_CHECK_LAUNCH(ctx, "gn_bwd_reduce");
    return DAT_OK;
}

int dat_gn_bwd_apply(dat_ctx* ctx, dat_stream s, int dtype, const void* g, const void* z, void* dz, const float* mean, const float* a,
                     const float* coef, int clips, long long rows, long long row_lo, long long nrows, int C, int cstride) {
    int rc = gn_check_shape(ctx, "gn_bwd_apply", dtype, clips, rows, C, cstride);
    if (rc != DAT_OK) return rc;
    rc = gn_check_window(ctx, "gn_bwd_apply", clips, rows, row_lo, nrows);
    if (rc != DAT_OK) return rc;
    DAT_ENFORCE(ctx, g && z && dz && mean && a && coef, "gn_bwd_apply: null argument");
    DAT_ENFORCE(ctx, aligned16(g) && aligned16(z) && aligned16(dz), "gn_bwd_apply: tensors must be 16-byte aligned");
    BN_LAUNCH(gn_bwd_apply_kernel, dim3(bn_row_blocks(dtype, rows, cstride), cstride / 64, clips), s, g, z, dz, mean, a, coef, rows, row_lo,
              nrows, C, cstride);
    DAT_CHECK_LAUNCH(ctx, "gn_bwd_apply");
    return DAT_OK;
}
