// SpatialBN (MODEL.USE_BN) on NDHWC blobs [rows][cstride]: batch statistics, normalise (+ residual, ReLU), and the two backward passes.
// DESIGN.md section 3.10.  Every kernel is bandwidth bound and shares one thread layout (the one of relu_bwd_kernel, train_ops.hip):
//
//   grid  = (row blocks, cstride / 64)          a block owns one 64-channel chunk of a strided set of rows
//   block = 256 threads = RL row lanes x TPR    TPR = 64 / VEC threads cover the chunk with ONE 16-byte access each
//                                               (fp32: VEC 4, TPR 16, RL 16;  16-bit: VEC 8, TPR 8, RL 32)
//
// so a thread keeps ONE channel group for the whole launch: its per-channel constants live in registers and its partial sums are per
// channel.  Reductions go thread -> LDS (fixed order over the row lanes) -> one partial row per block in the caller's workspace -> a
// finalize launch that merges the partial rows in a fixed order.  No float atomics anywhere: the same input gives the same bits.
// Padding channels [C, cstride) are written as zeros in every output and never enter a sum.
#include "dat_common.h"

namespace {

constexpr int BN_BLOCK = 256;
constexpr int BN_U = 4;                 // independent 16-byte loads in flight per thread and operand
constexpr int BN_MAX_BLOCKS = 1024;     // row blocks x channel chunks (four 256-thread blocks per CU)

template <int DT> struct Vec;
template <> struct Vec<DAT_F32> {
    static constexpr int N = 4;
    __device__ static __forceinline__ void ld(const void* p, size_t elem, float* v) {
        const float4 a = *(const float4*)((const float*)p + elem);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    }
    __device__ static __forceinline__ void st(void* p, size_t elem, const float* v) {
        *(float4*)((float*)p + elem) = make_float4(v[0], v[1], v[2], v[3]);
    }
};
template <> struct Vec<DAT_BF16> {
    static constexpr int N = 8;
    __device__ static __forceinline__ void ld(const void* p, size_t elem, float* v) {
        const uint4 a = *(const uint4*)((const uint16_t*)p + elem);
        const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = bf2f((uint16_t)(w[i] & 0xffffu));
            v[2 * i + 1] = bf2f((uint16_t)(w[i] >> 16));
        }
    }
    __device__ static __forceinline__ void st(void* p, size_t elem, const float* v) {
        uint4 a;
        a.x = f2bf2(v[0], v[1]); a.y = f2bf2(v[2], v[3]); a.z = f2bf2(v[4], v[5]); a.w = f2bf2(v[6], v[7]);
        *(uint4*)((uint16_t*)p + elem) = a;
    }
};

// the thread's place in the layout of the file comment
template <int DT> struct Lane {
    static constexpr int VEC = Vec<DT>::N, TPR = 64 / VEC, RL = BN_BLOCK / TPR;
    int c0, rl;                 // first channel of the thread's group, its row lane
    long long row0, step;       // first row, row step of the launch
    __device__ __forceinline__ Lane() {
        c0 = blockIdx.y * 64 + (threadIdx.x % TPR) * VEC;
        rl = threadIdx.x / TPR;
        row0 = (long long)blockIdx.x * RL + rl;
        step = (long long)gridDim.x * RL;
    }
};

// ---- forward: statistics --------------------------------------------------------------------------------------------------------
// per block and channel: (rows seen, their mean, M2 = sum (z - mean)^2).  Threads run Welford's update (one division per row, shared by the
// VEC channels), the row lanes of a block are merged with Chan's formula in lane order.
template <int DT>
__global__ void __launch_bounds__(BN_BLOCK) bn_stats_partial_kernel(const void* __restrict__ z, long long rows, int cs,
                                                                    float* __restrict__ pmean, float* __restrict__ pm2,
                                                                    float* __restrict__ pcnt) {
    typedef Lane<DT> L;
    constexpr int VEC = L::VEC;
    const L ln;
    float mean[VEC], m2[VEC], n = 0.f;
#pragma unroll
    for (int e = 0; e < VEC; ++e) mean[e] = m2[e] = 0.f;
    for (long long r = ln.row0; r < rows; r += ln.step * BN_U) {
        float v[BN_U][VEC];
#pragma unroll
        for (int u = 0; u < BN_U; ++u) {
            const long long rr = r + ln.step * u;
            Vec<DT>::ld(z, (size_t)(rr < rows ? rr : r) * cs + ln.c0, v[u]);
        }
#pragma unroll
        for (int u = 0; u < BN_U; ++u) {
            if (r + ln.step * u >= rows) break;
            n += 1.f;
            const float inv = 1.f / n;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float d = v[u][e] - mean[e];
                mean[e] += d * inv;
                m2[e] += d * (v[u][e] - mean[e]);
            }
        }
    }
    __shared__ float s_mean[BN_BLOCK * VEC], s_m2[BN_BLOCK * VEC], s_n[BN_BLOCK];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        s_mean[threadIdx.x * VEC + e] = mean[e];
        s_m2[threadIdx.x * VEC + e] = m2[e];
    }
    s_n[threadIdx.x] = n;
    __syncthreads();
    if (ln.rl != 0) return;
    for (int j = 1; j < L::RL; ++j) {
        const int t = j * L::TPR + threadIdx.x;
        const float nb = s_n[t];
        if (nb == 0.f) continue;
        const float nn = n + nb, f = nb / nn, g = n * f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float d = s_mean[t * VEC + e] - mean[e];
            mean[e] += d * f;
            m2[e] += s_m2[t * VEC + e] + d * d * g;
        }
        n = nn;
    }
    const size_t at = (size_t)blockIdx.x * cs + ln.c0;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        pmean[at + e] = mean[e];
        pm2[at + e] = m2[e];
    }
    if (threadIdx.x == 0) pcnt[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = n;
}

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

// ---- forward: y = act(z * a[c] + b'[c] (+ res)) ------------------------------------------------------------------------------------
template <int DT>
__global__ void __launch_bounds__(BN_BLOCK) bn_apply_kernel(const void* z, const void* res, void* y, const float* __restrict__ a,
                                                            const float* __restrict__ b, long long rows, int C, int cs, int relu) {
    typedef Lane<DT> L;
    constexpr int VEC = L::VEC;
    const L ln;
    float ka[VEC], kb[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        ka[e] = a[ln.c0 + e];
        kb[e] = b[ln.c0 + e];
    }
    for (long long r = ln.row0; r < rows; r += ln.step * BN_U) {
        float v[BN_U][VEC], q[BN_U][VEC];
#pragma unroll
        for (int u = 0; u < BN_U; ++u) {
            const long long rr = r + ln.step * u;
            const size_t at = (size_t)(rr < rows ? rr : r) * cs + ln.c0;
            Vec<DT>::ld(z, at, v[u]);
            if (res) Vec<DT>::ld(res, at, q[u]);
        }
#pragma unroll
        for (int u = 0; u < BN_U; ++u) {
            const long long rr = r + ln.step * u;
            if (rr >= rows) break;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                float o = fmaf(v[u][e], ka[e], kb[e]);
                if (res) o += q[u][e];
                if (relu) o = o > 0.f ? o : 0.f;
                v[u][e] = ln.c0 + e < C ? o : 0.f;
            }
            Vec<DT>::st(y, (size_t)rr * cs + ln.c0, v[u]);
        }
    }
}

// ---- backward: g = dy * [y > 0], per-block partial sums of g and g * xhat --------------------------------------------------------------
// dy / g hold the rows [row_lo, row_lo + nrows) of the blob; y and z point at the whole blob
template <int DT>
__global__ void __launch_bounds__(BN_BLOCK) bn_bwd_reduce_kernel(const void* dy, const void* __restrict__ y, const void* __restrict__ z,
                                                                 void* g, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                 long long row_lo, long long nrows, int C, int cs, int relu,
                                                                 float* __restrict__ pdb, float* __restrict__ pds) {
    typedef Lane<DT> L;
    constexpr int VEC = L::VEC;
    const L ln;
    float mu[VEC], rs[VEC], sb[VEC], ss[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        mu[e] = mean[ln.c0 + e];
        rs[e] = rstd[ln.c0 + e];
        sb[e] = ss[e] = 0.f;
    }
    for (long long r = ln.row0; r < nrows; r += ln.step * BN_U) {
        float d[BN_U][VEC], o[BN_U][VEC], x[BN_U][VEC];
#pragma unroll
        for (int u = 0; u < BN_U; ++u) {
            const long long rr = r + ln.step * u;
            const long long rc = rr < nrows ? rr : r;
            Vec<DT>::ld(dy, (size_t)rc * cs + ln.c0, d[u]);
            Vec<DT>::ld(z, (size_t)(row_lo + rc) * cs + ln.c0, x[u]);
            if (relu) Vec<DT>::ld(y, (size_t)(row_lo + rc) * cs + ln.c0, o[u]);
        }
#pragma unroll
        for (int u = 0; u < BN_U; ++u) {
            const long long rr = r + ln.step * u;
            if (rr >= nrows) break;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                float gv = d[u][e];
                if ((relu && !(o[u][e] > 0.f)) || ln.c0 + e >= C) gv = 0.f;
                d[u][e] = gv;
                sb[e] += gv;
                ss[e] += gv * ((x[u][e] - mu[e]) * rs[e]);
            }
            Vec<DT>::st(g, (size_t)rr * cs + ln.c0, d[u]);
        }
    }
    __shared__ float s_b[BN_BLOCK * VEC], s_s[BN_BLOCK * VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        s_b[threadIdx.x * VEC + e] = sb[e];
        s_s[threadIdx.x * VEC + e] = ss[e];
    }
    __syncthreads();
    if (ln.rl != 0) return;
    for (int j = 1; j < L::RL; ++j) {
        const int t = j * L::TPR + threadIdx.x;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            sb[e] += s_b[t * VEC + e];
            ss[e] += s_s[t * VEC + e];
        }
    }
    const size_t at = (size_t)blockIdx.x * cs + ln.c0;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        pdb[at + e] = sb[e];
        pds[at + e] = ss[e];
    }
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

// row blocks of a launch over `rows` rows: enough to fill the chip, few enough for a short finalize
int bn_row_blocks(int dtype, long long rows, int cs) {
    const int rl = dtype == DAT_BF16 ? Lane<DAT_BF16>::RL : Lane<DAT_F32>::RL;
    const int chunks = cs / 64;
    long long n = cdiv_ll(rows, (long long)rl * BN_U);
    const long long cap = BN_MAX_BLOCKS / chunks > 0 ? BN_MAX_BLOCKS / chunks : 1;
    if (n > cap) n = cap;
    return n < 1 ? 1 : (int)n;
}

size_t bn_ws_bytes(int dtype, long long rows, int cs) {
    return (size_t)bn_row_blocks(dtype, rows, cs) * (2 * (size_t)cs + cs / 64) * sizeof(float);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

size_t dat_bn_workspace_bytes(int dtype, long long rows, int cstride) {
    if (rows < 1 || cstride < 64 || cstride % 64 != 0) return 0;
    return bn_ws_bytes(dtype, rows, cstride);
}

#define BN_LAUNCH(kern, grid, s, ...)                                                                      \
    do {                                                                                                   \
        if (dtype == DAT_BF16) hipLaunchKernelGGL(kern<DAT_BF16>, grid, dim3(BN_BLOCK), 0, (hipStream_t)s, __VA_ARGS__); \
        else hipLaunchKernelGGL(kern<DAT_F32>, grid, dim3(BN_BLOCK), 0, (hipStream_t)s, __VA_ARGS__);        \
    } while (0)

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
    BN_LAUNCH(bn_stats_partial_kernel, dim3(nblk, chunks), s, z, rows, cstride, pmean, pm2, pcnt);
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
    BN_LAUNCH(bn_bwd_reduce_kernel, dim3(nblk, chunks), s, dy, y, z, g, mean, rstd, row_lo, nrows, C, cstride, relu, pdb, pds);
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
