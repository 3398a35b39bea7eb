// The thread layout and the three group-agnostic heavy kernels that SpatialBN (batch_norm.hip) and GroupNorm
// (group_norm.hip, section 3.11) share, on NDHWC blobs [clips][rows][cstride]:
//
//   grid  = (row blocks, cstride / 64, clips)   a block owns one 64-channel chunk of a strided set of rows of ONE clip
//   block = 256 threads = RL row lanes x TPR    TPR = 64 / VEC threads cover the chunk with ONE 16-byte access each
//                                               (fp32: VEC 4, TPR 16, RL 16;  16-bit: VEC 8, TPR 8, RL 32)
//
// so a thread keeps ONE channel group for the whole launch: its per-channel constants live in registers and its partial sums are per
// channel.  Reductions go thread -> LDS (fixed order over the row lanes) -> one partial row per block in the caller's workspace -> a
// finalize launch that merges the partial rows in a fixed order.  No float atomics anywhere: the same input gives the same bits.
// Padding channels [C, cstride) are written as zeros in every output and never enter a sum.
//
// The clip dimension: every per-channel table ([cstride] floats) and every partial row block is one of gridDim.z consecutive copies,
// one per clip, and a clip's blocks read that clip's rows only -- what a clip gets does not depend on how many clips the launch holds.
// SpatialBN launches with gridDim.z = 1 (its statistics span the whole blob).
#pragma once
#include "dat_common.h"

namespace {

constexpr int BN_BLOCK = 256;
constexpr int BN_U = 4;                 // independent 16-byte loads in flight per thread and operand
constexpr int BN_MAX_BLOCKS = 1024;     // row blocks x channel chunks (four 256-thread blocks per CU)

template <int DT> struct Vec;
template <> struct Vec<DAT_F32> {
    static constexpr int N = 4;
    // one 16-byte vector in registers <-> its N values
    __device__ static __forceinline__ void unpack(const uint4& a, float* v) {
        v[0] = __uint_as_float(a.x); v[1] = __uint_as_float(a.y); v[2] = __uint_as_float(a.z); v[3] = __uint_as_float(a.w);
    }
    __device__ static __forceinline__ uint4 pack(const float* v) {
        return make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
    }
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
    // one 16-byte vector in registers <-> its N values: the only copy of the 16-bit conversion of these kernels (ld / st go through it)
    __device__ static __forceinline__ void unpack(const uint4& a, float* v) {
        const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = bf2f((uint16_t)(w[i] & 0xffffu));
            v[2 * i + 1] = bf2f((uint16_t)(w[i] >> 16));
        }
    }
    __device__ static __forceinline__ uint4 pack(const float* v) {
        uint4 a;
        a.x = f2bf2(v[0], v[1]); a.y = f2bf2(v[2], v[3]); a.z = f2bf2(v[4], v[5]); a.w = f2bf2(v[6], v[7]);
        return a;
    }
    __device__ static __forceinline__ void ld(const void* p, size_t elem, float* v) { unpack(*(const uint4*)((const uint16_t*)p + elem), v); }
    __device__ static __forceinline__ void st(void* p, size_t elem, const float* v) { *(uint4*)((uint16_t*)p + elem) = pack(v); }
};

// the thread's place in the layout of the file comment
template <int DT> struct Lane {
    static constexpr int VEC = Vec<DT>::N, TPR = 64 / VEC, RL = BN_BLOCK / TPR;
    int c0, rl;                 // first channel of the thread's group, its row lane
    long long row0, step;       // first row, row step of the launch
    size_t clip;                // the block's clip
    __device__ __forceinline__ Lane() {
        c0 = blockIdx.y * 64 + (threadIdx.x % TPR) * VEC;
        rl = threadIdx.x / TPR;
        row0 = (long long)blockIdx.x * RL + rl;
        step = (long long)gridDim.x * RL;
        clip = blockIdx.z;
    }
};

// ---- forward: statistics --------------------------------------------------------------------------------------------------------
// per clip, block and channel: (rows seen, their mean, M2 = sum (z - mean)^2) over the `rows` rows of the clip.  Threads run Welford's
// update (one division per row, shared by the VEC channels), the row lanes of a block are merged with Chan's formula in lane order.
// pmean / pm2: [clips][row blocks][cs];  pcnt: [clips][chunks][row blocks].
// shift (NULL: none, SpatialBN): [clips][cs].  With it the statistics are those of z - K, K[clip][c] = the clip's FIRST row (written to
// `shift` for the finalize): an fp32 mean near 100 carries an absolute error of 4e-6, and Chan's merge turns the error of a difference
// of two such means into a first-order error of M2; the means of z - K are of the size of the spread, and so are their errors.
template <int DT>
__global__ void __launch_bounds__(BN_BLOCK) bn_stats_partial_kernel(const void* __restrict__ z, long long rows, int cs,
                                                                    float* __restrict__ pmean, float* __restrict__ pm2,
                                                                    float* __restrict__ pcnt, float* __restrict__ shift) {
    typedef Lane<DT> L;
    constexpr int VEC = L::VEC;
    const L ln;
    const size_t base = ln.clip * (size_t)rows * cs;
    float mean[VEC], m2[VEC], K[VEC], n = 0.f;
#pragma unroll
    for (int e = 0; e < VEC; ++e) mean[e] = m2[e] = K[e] = 0.f;
    if (shift) {
        Vec<DT>::ld(z, base + ln.c0, K);
        if (blockIdx.x == 0 && ln.rl == 0) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) shift[ln.clip * cs + ln.c0 + e] = K[e];
        }
    }
    for (long long r = ln.row0; r < rows; r += ln.step * BN_U) {
        float v[BN_U][VEC];
#pragma unroll
        for (int u = 0; u < BN_U; ++u) {
            const long long rr = r + ln.step * u;
            Vec<DT>::ld(z, base + (size_t)(rr < rows ? rr : r) * cs + ln.c0, v[u]);
        }
#pragma unroll
        for (int u = 0; u < BN_U; ++u) {
            if (r + ln.step * u >= rows) break;
            n += 1.f;
            const float inv = 1.f / n;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float x = v[u][e] - K[e];         // (K = 0 without a shift: x is v, bit for bit)
                const float d = x - mean[e];
                mean[e] += d * inv;
                m2[e] += d * (x - mean[e]);
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
    const size_t at = (ln.clip * gridDim.x + blockIdx.x) * cs + ln.c0;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        pmean[at + e] = mean[e];
        pm2[at + e] = m2[e];
    }
    if (threadIdx.x == 0) pcnt[(ln.clip * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = n;
}

// ---- forward: y = act(z * a[clip][c] + b'[clip][c] (+ res)) -----------------------------------------------------------------------
template <int DT>
__global__ void __launch_bounds__(BN_BLOCK) bn_apply_kernel(const void* z, const void* res, void* y, const float* __restrict__ a,
                                                            const float* __restrict__ b, long long rows, int C, int cs, int relu) {
    typedef Lane<DT> L;
    constexpr int VEC = L::VEC;
    const L ln;
    const size_t base = ln.clip * (size_t)rows * cs;
    float ka[VEC], kb[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        ka[e] = a[ln.clip * cs + ln.c0 + e];
        kb[e] = b[ln.clip * cs + ln.c0 + e];
    }
    for (long long r = ln.row0; r < rows; r += ln.step * BN_U) {
        float v[BN_U][VEC], q[BN_U][VEC];
#pragma unroll
        for (int u = 0; u < BN_U; ++u) {
            const long long rr = r + ln.step * u;
            const size_t at = base + (size_t)(rr < rows ? rr : r) * cs + ln.c0;
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
            Vec<DT>::st(y, base + (size_t)rr * cs + ln.c0, v[u]);
        }
    }
}

// ---- backward: g = dy * [y > 0], per-block partial sums of g and g * xhat --------------------------------------------------------------
// dy / g hold the rows [row_lo, row_lo + nrows) of every clip; y and z point at the whole blob, `rows` rows per clip
// (several clips: the window is the whole clip).  mean / rstd: [clips][cs];  pdb / pds: [clips][row blocks][cs].
template <int DT>
__global__ void __launch_bounds__(BN_BLOCK) bn_bwd_reduce_kernel(const void* dy, const void* __restrict__ y, const void* __restrict__ z,
                                                                 void* g, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                 long long rows, long long row_lo, long long nrows, int C, int cs, int relu,
                                                                 float* __restrict__ pdb, float* __restrict__ pds) {
    typedef Lane<DT> L;
    constexpr int VEC = L::VEC;
    const L ln;
    const size_t wbase = ln.clip * (size_t)nrows * cs, zbase = (ln.clip * (size_t)rows + row_lo) * cs;
    float mu[VEC], rs[VEC], sb[VEC], ss[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        mu[e] = mean[ln.clip * cs + ln.c0 + e];
        rs[e] = rstd[ln.clip * cs + ln.c0 + e];
        sb[e] = ss[e] = 0.f;
    }
    for (long long r = ln.row0; r < nrows; r += ln.step * BN_U) {
        float d[BN_U][VEC], o[BN_U][VEC], x[BN_U][VEC];
#pragma unroll
        for (int u = 0; u < BN_U; ++u) {
            const long long rr = r + ln.step * u;
            const long long rc = rr < nrows ? rr : r;
            Vec<DT>::ld(dy, wbase + (size_t)rc * cs + ln.c0, d[u]);
            Vec<DT>::ld(z, zbase + (size_t)rc * cs + ln.c0, x[u]);
            if (relu) Vec<DT>::ld(y, zbase + (size_t)rc * cs + ln.c0, o[u]);
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
            Vec<DT>::st(g, wbase + (size_t)rr * cs + ln.c0, d[u]);
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
    const size_t at = (ln.clip * gridDim.x + blockIdx.x) * cs + ln.c0;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        pdb[at + e] = sb[e];
        pds[at + e] = ss[e];
    }
}

// row blocks of a launch over `rows` rows (of one clip): enough to fill the chip, few enough for a short finalize.  A function of the
// clip's own shape only, never of the number of clips: the merge order, and with it every bit of a clip's statistics, stays the same.
int bn_row_blocks(int dtype, long long rows, int cs) {
    const int rl = dtype == DAT_BF16 ? Lane<DAT_BF16>::RL : Lane<DAT_F32>::RL;
    const int chunks = cs / 64;
    long long n = cdiv_ll(rows, (long long)rl * BN_U);
    const long long cap = BN_MAX_BLOCKS / chunks > 0 ? BN_MAX_BLOCKS / chunks : 1;
    if (n > cap) n = cap;
    return n < 1 ? 1 : (int)n;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

#define BN_LAUNCH(kern, grid, s, ...)                                                                      \
    do {                                                                                                   \
        if (dtype == DAT_BF16) hipLaunchKernelGGL(kern<DAT_BF16>, grid, dim3(BN_BLOCK), 0, (hipStream_t)s, __VA_ARGS__); \
        else hipLaunchKernelGGL(kern<DAT_F32>, grid, dim3(BN_BLOCK), 0, (hipStream_t)s, __VA_ARGS__);        \
    } while (0)
