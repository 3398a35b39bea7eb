// SpatialBN (MODEL.USE_BN) on NDHWC blobs [rows][cstride]: batch statistics, normalise (+ residual, ReLU), and the two backward passes.
// DESIGN.md section 3.10.  Every kernel is bandwidth bound and shares one thread layout (the one of relu_bwd_kernel, train_ops.hip):
// The thread layout, the statistics, apply and backward-reduce kernels are in norm_kernels.h (shared with group_norm.hip); this file
// holds what knows that the statistics are per channel over the whole blob: the two finalize kernels and the backward apply.
#include "norm_kernels.h"

namespace {

// one block per 64-channel chunk, 4 lanes per channel: each lane merges every fourth partial row in order, lane 0 merges the four.
// Writes the saved mean / rstd, the folded pair a = s * rstd, b' = b - mean * a (zeros in the padding channels) and updates the running
// statistics in place: rm = m * rm + (1 - m) * mean, riv = m * riv + (1 - m) * M2 / (M - 1)  (a running VARIANCE, unbiased).
__global__ void __launch_bounds__(BN_BLOCK) bn_stats_finalize_kernel(const float* __restrict__ pmean, const float* __restrict__ pm2,
                                                                     const float* __restrict__ pcnt, int nblk, int cs, int C, long long rows,
                                                                     const float* __restrict__ scale, const float* __restrict__ bias, float eps,
                                                                     float momentum, float* __restrict__ rm, float* __restrict__ riv,
                                                                     float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                                     float* __restrict__ a_out, float* __restrict__ b_out) {
    const int cl = threadIdx.x & 63, lane = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    float n = 0.f, mean = 0.f, m2 = 0.f;
    for (int b = lane; b < nblk; b += 4) {
        const float nb = pcnt[(size_t)blockIdx.x * nblk + b];
        if (nb == 0.f) continue;
        const float mb = pmean[(size_t)b * cs + c], qb = pm2[(size_t)b * cs + c];
        const float nn = n + nb, f = nb / nn, d = mb - mean;
        mean += d * f;
        m2 += qb + d * d * (n * f);
        n = nn;
    }
    __shared__ float s[3][BN_BLOCK];
    s[0][threadIdx.x] = n; s[1][threadIdx.x] = mean; s[2][threadIdx.x] = m2;
    __syncthreads();
    if (lane != 0) return;
    for (int j = 1; j < 4; ++j) {
        const float nb = s[0][j * 64 + cl];
        if (nb == 0.f) continue;
        const float nn = n + nb, f = nb / nn, d = s[1][j * 64 + cl] - mean;
        mean += d * f;
        m2 += s[2][j * 64 + cl] + d * d * (n * f);
        n = nn;
    }
    if (c >= C) {
        mean_out[c] = rstd_out[c] = a_out[c] = b_out[c] = 0.f;
        return;
    }
    const float M = (float)rows;
    const float var = m2 / M;
    const float rstd = 1.f / sqrtf(var + eps);
    const float a = scale[c] * rstd;
    mean_out[c] = mean;
    rstd_out[c] = rstd;
    a_out[c] = a;
    b_out[c] = bias[c] - mean * a;
    if (rm) rm[c] = momentum * rm[c] + (1.f - momentum) * mean;
    if (riv) riv[c] = momentum * riv[c] + (1.f - momentum) * (m2 / (M - 1.f));
}

// sums[0][c] = sum g, sums[1][c] = sum g * xhat of THIS call (zeros in the padding channels); dbeta / dgamma (NULL: not trainable) accumulate
__global__ void __launch_bounds__(BN_BLOCK) bn_bwd_finalize_kernel(const float* __restrict__ pdb, const float* __restrict__ pds, int nblk,
                                                                   int cs, int C, float* __restrict__ sums, float* __restrict__ dbeta,
                                                                   float* __restrict__ dgamma) {
    const int cl = threadIdx.x & 63, lane = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    float b = 0.f, s = 0.f;
    for (int k = lane; k < nblk; k += 4) {
        b += pdb[(size_t)k * cs + c];
        s += pds[(size_t)k * cs + c];
    }
    __shared__ float sh[2][BN_BLOCK];
    sh[0][threadIdx.x] = b; sh[1][threadIdx.x] = s;
    __syncthreads();
    if (lane != 0) return;
    for (int j = 1; j < 4; ++j) {
        b += sh[0][j * 64 + cl];
        s += sh[1][j * 64 + cl];
    }
    if (c >= C) b = s = 0.f;
    sums[c] = b;
    sums[cs + c] = s;
    if (c < C) {
        if (dbeta) dbeta[c] += b;
        if (dgamma) dgamma[c] += s;
    }
}

// ---- backward: dz = a * (g - db / M - xhat * ds / M) on EVERY row of the blob (g = 0 outside [row_lo, row_lo + nrows)) ---------------
template <int DT>
__global__ void __launch_bounds__(BN_BLOCK) bn_bwd_apply_kernel(const void* __restrict__ g, const void* __restrict__ z, void* __restrict__ dz,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                const float* __restrict__ a, const float* __restrict__ sums,
                                                                long long rows, long long row_lo, long long nrows, int C, int cs) {
    typedef Lane<DT> L;
    constexpr int VEC = L::VEC;
    const L ln;
    const float invM = 1.f / (float)rows;
    float mu[VEC], rs[VEC], ka[VEC], kb[VEC], ks[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        mu[e] = mean[ln.c0 + e];
        rs[e] = rstd[ln.c0 + e];
        ka[e] = a[ln.c0 + e];
        kb[e] = sums[ln.c0 + e] * invM;
        ks[e] = sums[cs + ln.c0 + e] * invM;
    }
    for (long long r = ln.row0; r < rows; r += ln.step * BN_U) {
        float x[BN_U][VEC], gv[BN_U][VEC];
#pragma unroll
        for (int u = 0; u < BN_U; ++u) {
            const long long rr = r + ln.step * u;
            const long long rc = rr < rows ? rr : r;
            Vec<DT>::ld(z, (size_t)rc * cs + ln.c0, x[u]);
            const long long w = rc - row_lo;
            if (w >= 0 && w < nrows) {
                Vec<DT>::ld(g, (size_t)w * cs + ln.c0, gv[u]);
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
                const float xh = (x[u][e] - mu[e]) * rs[e];
                const float o = ka[e] * (gv[u][e] - kb[e] - xh * ks[e]);
                x[u][e] = ln.c0 + e < C ? o : 0.f;
            }
            Vec<DT>::st(dz, (size_t)rr * cs + ln.c0, x[u]);
        }
    }
}

size_t bn_ws_bytes(int dtype, long long rows, int cs) {
    return (size_t)bn_row_blocks(dtype, rows, cs) * (2 * (size_t)cs + cs / 64) * sizeof(float);
}

}  // namespace

size_t dat_bn_workspace_bytes(int dtype, long long rows, int cstride) {
    if (rows < 1 || cstride < 64 || cstride % 64 != 0) return 0;
    return bn_ws_bytes(dtype, rows, cstride);
}

static int bn_check_shape(dat_ctx* ctx, const char* what, int dtype, long long rows, int C, int cs) {
    DAT_ENFORCE(ctx, dtype == DAT_F32 || dtype == DAT_BF16, "%s: dtype %d", what, dtype);
    DAT_ENFORCE(ctx, rows >= 1 && rows * (long long)cs < (1ll << 40), "%s: %lld rows", what, rows);
    DAT_ENFORCE(ctx, cs >= 64 && cs % 64 == 0 && C >= 1 && C <= cs, "%s: %d channels at stride %d (a multiple of 64)", what, C, cs);
    return DAT_OK;
}

int dat_bn_stats(dat_ctx* ctx, dat_stream s, int dtype, const void* z, long long rows, int C, int cstride, const float* scale,
                 const float* bias, float eps, float momentum, float* rm, float* riv, float* mean, float* rstd, float* a, float* bprime,
                 void* ws, size_t ws_bytes) {
    int rc = bn_check_shape(ctx, "bn_stats", dtype, rows, C, cstride);
    if (rc != DAT_OK) return rc;
    DAT_ENFORCE(ctx, rows >= 2, "bn_stats: batch statistics need at least 2 positions per channel (got %lld)", rows);
    DAT_ENFORCE(ctx, z && scale && bias && mean && rstd && a && bprime && ws, "bn_stats: null argument");
    DAT_ENFORCE(ctx, aligned16(z), "bn_stats: z must be 16-byte aligned");
    DAT_ENFORCE(ctx, ws_bytes >= bn_ws_bytes(dtype, rows, cstride), "bn_stats: workspace of %zu bytes, %zu needed", ws_bytes,
                bn_ws_bytes(dtype, rows, cstride));
    const int nblk = bn_row_blocks(dtype, rows, cstride), chunks = cstride / 64;
    float* pmean = (float*)ws;
    float* pm2 = pmean + (size_t)nblk * cstride;
    float* pcnt = pm2 + (size_t)nblk * cstride;
    BN_LAUNCH(bn_stats_partial_kernel, dim3(nblk, chunks), s, z, rows, cstride, pmean, pm2, pcnt, (float*)nullptr);
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(chunks), dim3(BN_BLOCK), 0, (hipStream_t)s, (const float*)pmean, (const float*)pm2,
                       (const float*)pcnt, nblk, cstride, C, rows, scale, bias, eps, momentum, rm, riv, mean, rstd, a, bprime);
    DAT_CHECK_LAUNCH(ctx, "bn_stats");
    return DAT_OK;
}

int dat_bn_apply(dat_ctx* ctx, dat_stream s, int dtype, const void* z, const void* residual, void* y, const float* a, const float* bprime,
                 long long rows, int C, int cstride, int relu) {
    int rc = bn_check_shape(ctx, "bn_apply", dtype, rows, C, cstride);
    if (rc != DAT_OK) return rc;
    DAT_ENFORCE(ctx, z && y && a && bprime, "bn_apply: null argument");
    DAT_ENFORCE(ctx, aligned16(z) && aligned16(y) && aligned16(residual), "bn_apply: tensors must be 16-byte aligned");
    BN_LAUNCH(bn_apply_kernel, dim3(bn_row_blocks(dtype, rows, cstride), cstride / 64), s, z, residual, y, a, bprime, rows, C, cstride,
              relu);
    DAT_CHECK_LAUNCH(ctx, "bn_apply");
    return DAT_OK;
}

int dat_bn_bwd_reduce(dat_ctx* ctx, dat_stream s, int dtype, const void* dy, const void* y, const void* z, void* g, const float* mean,
                      const float* rstd, long long rows, long long row_lo, long long nrows, int C, int cstride, int relu, float* sums,
                      float* dbeta, float* dgamma, void* ws, size_t ws_bytes) {
    int rc = bn_check_shape(ctx, "bn_bwd_reduce", dtype, rows, C, cstride);
    if (rc != DAT_OK) return rc;
    DAT_ENFORCE(ctx, row_lo >= 0 && nrows >= 1 && row_lo + nrows <= rows, "bn_bwd_reduce: window [%lld, %lld) of %lld rows", row_lo,
                row_lo + nrows, rows);
    DAT_ENFORCE(ctx, dy && z && g && mean && rstd && sums && ws && (y || !relu), "bn_bwd_reduce: null argument");
    DAT_ENFORCE(ctx, aligned16(dy) && aligned16(y) && aligned16(z) && aligned16(g), "bn_bwd_reduce: tensors must be 16-byte aligned");
    DAT_ENFORCE(ctx, ws_bytes >= bn_ws_bytes(dtype, nrows, cstride), "bn_bwd_reduce: workspace of %zu bytes, %zu needed", ws_bytes,
                bn_ws_bytes(dtype, nrows, cstride));
    const int nblk = bn_row_blocks(dtype, nrows, cstride), chunks = cstride / 64;
    float* pdb = (float*)ws;
    float* pds = pdb + (size_t)nblk * cstride;
    BN_LAUNCH(bn_bwd_reduce_kernel, dim3(nblk, chunks), s, dy, y, z, g, mean, rstd, rows, row_lo, nrows, C, cstride, relu, pdb, pds);
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(chunks), dim3(BN_BLOCK), 0, (hipStream_t)s, (const float*)pdb, (const float*)pds, nblk,
                       cstride, C, sums, dbeta, dgamma);
    DAT_CHECK_LAUNCH(ctx, "bn_bwd_reduce");
    return DAT_OK;
}

int dat_bn_bwd_apply(dat_ctx* ctx, dat_stream s, int dtype, const void* g, const void* z, void* dz, const float* mean, const float* rstd,
                     const float* a, const float* sums, long long rows, long long row_lo, long long nrows, int C, int cstride) {
    int rc = bn_check_shape(ctx, "bn_bwd_apply", dtype, rows, C, cstride);
    if (rc != DAT_OK) return rc;
    DAT_ENFORCE(ctx, rows >= 2, "bn_bwd_apply: batch statistics need at least 2 positions per channel (got %lld)", rows);
    DAT_ENFORCE(ctx, row_lo >= 0 && nrows >= 1 && row_lo + nrows <= rows, "bn_bwd_apply: window [%lld, %lld) of %lld rows", row_lo,
                row_lo + nrows, rows);
    DAT_ENFORCE(ctx, g && z && dz && mean && rstd && a && sums, "bn_bwd_apply: null argument");
    DAT_ENFORCE(ctx, aligned16(g) && aligned16(z) && aligned16(dz), "bn_bwd_apply: tensors must be 16-byte aligned");
    BN_LAUNCH(bn_bwd_apply_kernel, dim3(bn_row_blocks(dtype, rows, cstride), cstride / 64), s, g, z, dz, mean, rstd, a, sums, rows, row_lo,
              nrows, C, cstride);
    DAT_CHECK_LAUNCH(ctx, "bn_bwd_apply");
    return DAT_OK;
}
