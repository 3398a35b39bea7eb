// Backward of the spacetime non-local block's fused attention (HIP.TRAIN_NONLOCAL) and of its 2 x 2 max-pool.
//
// With lse_i the row statistic of the training forward (dat_nonlocal_attention_lse), c = scale * log2(e) and
//     p_ij = exp2(c s_ij - lse_i),   delta_i = sum_d dy_id y_id,   dP_ij = sum_d dy_id v_jd,   dS_ij = p_ij (dP_ij - delta_i)
// the gradients are  dv_jd = sum_i p_ij dy_id,  dq_id = scale sum_j dS_ij k_jd,  dk_jd = scale sum_i dS_ij q_id.  P is recomputed tile by tile:
// the [Lq, Lk] scores never reach memory.  Three launches, none of which adds across workgroups -- no float atomics, no hand-off between
// workgroups, no host synchronisation, so the result is bitwise reproducible and does not depend on the number of clips:
//   * nl_delta_kernel: delta in fp32, one value per query row, stored next to lse;
//   * nl_bwd_dq_kernel, QUERY-stationary and shaped like the forward: a wave owns 32 query rows (q and dy fragments in registers), the
//     workgroup walks the key tiles.  S^T = K Q^T and dP^T = V dY^T have the query on the lane, so lse and delta are per-lane scalars and
//     the dS^T accumulator tile is the B operand of dQ^T += K^T dS^T (K^T read from a transposed LDS image in the forward's k order);
//   * nl_bwd_dkdv_kernel, KEY-stationary: a wave owns 32 keys (k and v fragments in registers), the workgroup walks the query tiles.
//     S = Q K^T and dP = dY V^T have the key on the lane; P and dS are the B operands of dV^T += dY^T P and dK^T += Q^T dS.
// That is seven MFMA products per pair of tiles instead of five.  Where the accumulators do not fit (D = 512, fp32 at D >= 256) a launch
// works on output-channel slices (blockIdx.z) and recomputes the scores per slice, as the forward does at D = 512.
//
// Numerics: fp32 accumulation everywhere; c applied in fp32 to the accumulated score; P and dS rounded to nearest once for the 16-bit
// MFMAs; scale applied in fp32 to the accumulated dq / dk; each output rounded once.  Rows at or past Lq / Lk are zero-filled in LDS and
// their p is SET to zero (not computed), so they contribute exactly zero; a zero-filled row uses lse = delta = 0.
#include "dat_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2_t;

constexpr int NB_ROWS = 128;   // stationary rows per workgroup (4 waves x 32)
constexpr int NB_T = 32;       // streamed rows per tile
constexpr int NB_TSTR = 36;    // row stride of a transposed 16-bit image [channel][32 rows + 8 bytes]

struct NbParams {
    const void *q, *k, *v, *dy;
    const float *lse, *delta;
    void *dq, *dk, *dv;
    long long Lq, Lk;
    int ldq, ldk, ldv, lddy, lddq, lddk, lddv;
    float c;       // scale * log2(e)
    float scale;
};

template <int DT, int D, int DV>
struct NbCfg {
    static constexpr int ES = DT == DAT_BF16 ? 2 : 4;
    // row-major image [32 rows][STR]: 16-bit rows padded by 16 bytes, fp32 rows by 2 floats (nonlocal.hip NlCfg::KSTR)
    static constexpr int STR = DT == DAT_BF16 ? D + 8 : D + 2;
    static constexpr int ROW_BYTES = NB_T * STR * ES;
    static constexpr int TR_BYTES = DT == DAT_BF16 ? DV * NB_TSTR * 2 : 0;   // fp32 reads the row-major image by columns instead
    static constexpr int NQ = DT == DAT_BF16 ? D / 16 * 4 : D / 2;           // registers of a lane's stationary fragments (one operand)
    static constexpr bool REG = 2 * NQ <= 256;                               // both stationary operands live in registers
    static constexpr bool PREF = DT == DAT_BF16 && D <= 128;                 // the next tile's loads wait in registers under this tile's MFMAs
    static constexpr int DQ_LDS = 2 * ROW_BYTES + TR_BYTES;                  // K, V, K^T slice
    static constexpr int DKDV_LDS = 2 * ROW_BYTES + 2 * TR_BYTES + 2 * NB_T * 4;   // Q, dY, Q^T and dY^T slices, lse, delta
};

__device__ __forceinline__ int nb_crow(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// rows [row0, row0 + 32) of src (channels [0, D)) -> dst [32][STR]; rows at or past `limit` are zero
template <int DT, int D, int STR>
__device__ __forceinline__ void nb_stage_rows(typename ElemOf<DT>::type* dst, const typename ElemOf<DT>::type* src, int ld, long long row0,
                                              long long limit, int tid) {
    if constexpr (DT == DAT_BF16) {
        for (int c = tid; c < NB_T * (D / 8); c += 256) {
            const int row = c / (D / 8), c8 = c % (D / 8);
            u32x4_t t = {0u, 0u, 0u, 0u};
            if (row0 + row < limit) t = *(const u32x4_t*)(src + (size_t)(row0 + row) * ld + c8 * 8);
            *(u32x4_t*)(dst + row * STR + c8 * 8) = t;
        }
    } else {
        for (int c = tid; c < NB_T * (D / 4); c += 256) {
            const int row = c / (D / 4), c4 = c % (D / 4);
            u32x4_t t = {0u, 0u, 0u, 0u};
            if (row0 + row < limit) t = *(const u32x4_t*)(src + (size_t)(row0 + row) * ld + c4 * 4);
            u32x2_t* o = (u32x2_t*)(dst + row * STR + c4 * 4);   // rows are 8-byte aligned only
            o[0] = u32x2_t{t.x, t.y};
            o[1] = u32x2_t{t.z, t.w};
        }
    }
}

// 16-bit: the same rows, channels [0, DV) of src, TRANSPOSED -> dst [DV][36]: one item = two adjacent rows x 8 channels -> 8 dword stores
template <int DV>
__device__ __forceinline__ void nb_stage_tr(uint16_t* dst, const uint16_t* src, int ld, long long row0, long long limit, int tid) {
    for (int c = tid; c < (NB_T / 2) * (DV / 8); c += 256) {
        const int kp = c / (DV / 8), c8 = c % (DV / 8);
        u32x4_t a = {0u, 0u, 0u, 0u}, b = {0u, 0u, 0u, 0u};
        if (row0 + 2 * kp < limit) a = *(const u32x4_t*)(src + (size_t)(row0 + 2 * kp) * ld + c8 * 8);
        if (row0 + 2 * kp + 1 < limit) b = *(const u32x4_t*)(src + (size_t)(row0 + 2 * kp + 1) * ld + c8 * 8);
        uint32_t* o = (uint32_t*)(dst + (c8 * 8) * NB_TSTR + 2 * kp);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t wa = a[i], wb = b[i];
            o[(2 * i) * (NB_TSTR / 2)] = (wa & 0xffffu) | (wb << 16);
            o[(2 * i + 1) * (NB_TSTR / 2)] = (wa >> 16) | (wb & 0xffff0000u);
        }
    }
}

// 16-bit, D <= 128: a thread's share of a streamed tile on its way from memory to LDS.  The loads of tile t + 1 are issued before the MFMAs of
// tile t and stay in flight under them (at one wave per SIMD nothing else hides the latency of a tile's loads); `store` writes the images
// nb_stage_rows / nb_stage_tr write.  (D >= 256 has no registers left for it.)
template <int D, int STR>
struct NbRowRegs {
    static constexpr int N = D / 64;   // 16-byte chunks per thread: 32 * (D / 8) / 256
    u32x4_t r[N];
    __device__ __forceinline__ void load(const uint16_t* src, int ld, long long row0, long long limit, int tid) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int c = tid + i * 256, row = c / (D / 8), c8 = c % (D / 8);
            r[i] = u32x4_t{0u, 0u, 0u, 0u};
            if (row0 + row < limit) r[i] = *(const u32x4_t*)(src + (size_t)(row0 + row) * ld + c8 * 8);
        }
    }
    __device__ __forceinline__ void store(uint16_t* dst, int tid) const {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int c = tid + i * 256, row = c / (D / 8), c8 = c % (D / 8);
            *(u32x4_t*)(dst + row * STR + c8 * 8) = r[i];
        }
    }
};

template <int DV>
struct NbTrRegs {
    static_assert((NB_T / 2) * (DV / 8) <= 256, "one item per thread");
    u32x4_t a, b;
    __device__ __forceinline__ void load(const uint16_t* src, int ld, long long row0, long long limit, int tid) {
        const int kp = tid / (DV / 8), c8 = tid % (DV / 8);
        a = b = u32x4_t{0u, 0u, 0u, 0u};
        if (tid < (NB_T / 2) * (DV / 8)) {
            if (row0 + 2 * kp < limit) a = *(const u32x4_t*)(src + (size_t)(row0 + 2 * kp) * ld + c8 * 8);
            if (row0 + 2 * kp + 1 < limit) b = *(const u32x4_t*)(src + (size_t)(row0 + 2 * kp + 1) * ld + c8 * 8);
        }
    }
    __device__ __forceinline__ void store(uint16_t* dst, int tid) const {
        const int kp = tid / (DV / 8), c8 = tid % (DV / 8);
        if (tid < (NB_T / 2) * (DV / 8)) {
            uint32_t* o = (uint32_t*)(dst + (c8 * 8) * NB_TSTR + 2 * kp);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t wa = a[i], wb = b[i];
                o[(2 * i) * (NB_TSTR / 2)] = (wa & 0xffffu) | (wb << 16);
                o[(2 * i + 1) * (NB_TSTR / 2)] = (wa >> 16) | (wb & 0xffff0000u);
            }
        }
    }
};

// a lane's fragments of one row (the B operand of the two row-major products): 16-bit k step s takes channels 16 s + 8 h + (0 .. 7), fp32
// k step s takes channel 2 s + h
template <int DT, int D, int NQ>
__device__ __forceinline__ void nb_load_frag(uint32_t (&f)[NQ], const typename ElemOf<DT>::type* row, bool valid, int h) {
    if constexpr (DT == DAT_BF16) {
#pragma unroll
        for (int s = 0; s < D / 16; ++s) {
            u32x4_t t = {0u, 0u, 0u, 0u};
            if (valid) t = *(const u32x4_t*)(row + 16 * s + 8 * h);
            f[4 * s] = t.x; f[4 * s + 1] = t.y; f[4 * s + 2] = t.z; f[4 * s + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int s = 0; s < D / 2; ++s) f[s] = valid ? ((const uint32_t*)row)[2 * s + h] : 0u;
    }
}

// acc += A B^T over the D channels: A = rows of the LDS image (lane r: row r), B = the lane's stationary row (registers, or memory when
// the fragments of two operands do not fit: the fp32 parity path at D = 512)
template <int DT, int D, int STR, int NQ, bool REG>
__device__ __forceinline__ f32x16_t nb_row_product(const typename ElemOf<DT>::type* img, const uint32_t (&f)[REG ? NQ : 1],
                                                   const typename ElemOf<DT>::type* brow, bool bvalid, int r, int h) {
    f32x16_t acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    if constexpr (DT == DAT_BF16) {
        static_assert(REG, "16-bit fragments always fit");
#pragma unroll
        for (int s = 0; s < D / 16; ++s) {
            const u32x4_t a = *(const u32x4_t*)(img + r * STR + 16 * s + 8 * h);
            const u32x4_t b = {f[4 * s], f[4 * s + 1], f[4 * s + 2], f[4 * s + 3]};
            acc = DAT_MFMA16(a, b, acc);
        }
    } else {
        if constexpr (REG) {
#pragma unroll
            for (int s = 0; s < D / 2; ++s)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(img[r * STR + 2 * s + h], __uint_as_float(f[s]), acc, 0, 0, 0);
        } else {
#pragma unroll 16
            for (int s = 0; s < D / 2; ++s)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(img[r * STR + 2 * s + h], bvalid ? brow[2 * s + h] : 0.f, acc, 0, 0, 0);
        }
    }
    return acc;
}

// acc[n] += A^T B over the 32 rows of a tile: A^T = channels [ch0 + 32 n, + 32) of the tile (16-bit: the transposed image `tr`, whose
// channel 0 is ch0; fp32: the row-major image read by columns), B = t[16], this lane's accumulator tile of the previous product
template <int DT, int DV, int STR>
__device__ __forceinline__ void nb_col_product(f32x16_t (&acc)[DV / 32], const typename ElemOf<DT>::type* tr,
                                               const typename ElemOf<DT>::type* img, int ch0, const float (&t)[16], int r, int h) {
    if constexpr (DT == DAT_BF16) {
        u32x4_t pb[2];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int i = 0; i < 4; ++i) pb[s][i] = f2bf2(t[8 * s + 2 * i], t[8 * s + 2 * i + 1]);   // round to nearest even, once
#pragma unroll
        for (int n = 0; n < DV / 32; ++n) {
            const uint16_t* row = tr + (n * 32 + r) * NB_TSTR;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const u32x2_t lo = *(const u32x2_t*)(row + 16 * s + 4 * h);
                const u32x2_t hi = *(const u32x2_t*)(row + 16 * s + 8 + 4 * h);
                const u32x4_t a = {lo.x, lo.y, hi.x, hi.y};
                acc[n] = DAT_MFMA16(a, pb[s], acc[n]);
            }
        }
    } else {
#pragma unroll
        for (int n = 0; n < DV / 32; ++n)
#pragma unroll
            for (int i = 0; i < 16; ++i)
                acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(img[nb_crow(i, h) * STR + ch0 + n * 32 + r], t[i], acc[n], 0, 0, 0);
    }
}

// out[row][ch0 + ...] = mult * acc^T: registers 4 g .. 4 g + 3 of tile n are channels n * 32 + 8 g + 4 h + (0 .. 3) of the lane's row
template <int DT, int DV>
__device__ __forceinline__ void nb_store(typename ElemOf<DT>::type* dst, const f32x16_t (&acc)[DV / 32], float mult, int h) {
#pragma unroll
    for (int n = 0; n < DV / 32; ++n)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float o0 = acc[n][4 * g] * mult, o1 = acc[n][4 * g + 1] * mult, o2 = acc[n][4 * g + 2] * mult, o3 = acc[n][4 * g + 3] * mult;
            typename ElemOf<DT>::type* o = dst + n * 32 + 8 * g + 4 * h;
            if constexpr (DT == DAT_BF16)
                *(u32x2_t*)o = u32x2_t{f2bf2(o0, o1), f2bf2(o2, o3)};
            else
                *(f32x4_t*)o = f32x4_t{o0, o1, o2, o3};
        }
}

// delta[row] = sum_d dy y in fp32: 16 lanes per row, a fixed reduction order
template <int DT>
__global__ __launch_bounds__(256) void nl_delta_kernel(const void* __restrict__ y, const void* __restrict__ dy, float* __restrict__ delta,
                                                       long long rows, int D, int ldy, int lddy) {
    const long long row = ((long long)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int sub = threadIdx.x & 15;
    float acc = 0.f;
    if (row < rows)
        for (int d = sub; d < D; d += 16) acc += ElemOf<DT>::ld(dy, (size_t)row * lddy + d) * ElemOf<DT>::ld(y, (size_t)row * ldy + d);
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
    if (row < rows && sub == 0) delta[row] = acc;
}

template <int DT, int D, int DV>
__global__ __launch_bounds__(256) void nl_bwd_dq_kernel(NbParams p) {
    typedef NbCfg<DT, D, DV> Cfg;
    typedef typename ElemOf<DT>::type T;
    extern __shared__ __align__(16) unsigned char nb_smem[];
    T* Ks = (T*)nb_smem;
    T* Vs = (T*)(nb_smem + Cfg::ROW_BYTES);
    T* Kt = (T*)(nb_smem + 2 * Cfg::ROW_BYTES);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const long long clip = blockIdx.y;
    const long long q0 = (long long)blockIdx.x * NB_ROWS + wave * 32;
    const int dv0 = (int)blockIdx.z * DV;
    const long long qrow = q0 + r;
    const bool qvalid = qrow < p.Lq;
    const bool wave_active = q0 < p.Lq;   // wave-uniform: a wave past the last row still stages tiles and meets the barriers

    const T* kbase = (const T*)p.k + (size_t)(clip * p.Lk) * p.ldk;
    const T* vbase = (const T*)p.v + (size_t)(clip * p.Lk) * p.ldv;
    const size_t grow = (size_t)(clip * p.Lq + (qvalid ? qrow : 0));
    const T* qp = (const T*)p.q + grow * p.ldq;
    const T* dyp = (const T*)p.dy + grow * p.lddy;
    const float lse_i = qvalid ? p.lse[grow] : 0.f;
    const float del_i = qvalid ? p.delta[grow] : 0.f;

    uint32_t qf[Cfg::REG ? Cfg::NQ : 1], dyf[Cfg::REG ? Cfg::NQ : 1];
    if constexpr (Cfg::REG) {
        nb_load_frag<DT, D, Cfg::NQ>(qf, qp, qvalid, h);
        nb_load_frag<DT, D, Cfg::NQ>(dyf, dyp, qvalid, h);
    }

    f32x16_t acc[DV / 32];
#pragma unroll
    for (int n = 0; n < DV / 32; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[n][i] = 0.f;

    constexpr bool PREF = Cfg::PREF;
    NbRowRegs<PREF ? D : 64, Cfg::STR> kregs, vregs;
    NbTrRegs<PREF ? DV : 64> ktregs;
    auto load_tile = [&](long long key0) {
        kregs.load((const uint16_t*)kbase, p.ldk, key0, p.Lk, tid);
        vregs.load((const uint16_t*)vbase, p.ldv, key0, p.Lk, tid);
        ktregs.load((const uint16_t*)kbase + dv0, p.ldk, key0, p.Lk, tid);
    };
    const long long ntiles = (p.Lk + NB_T - 1) / NB_T;
    if constexpr (PREF) load_tile(0);
    for (long long kt = 0; kt < ntiles; ++kt) {
        const long long key0 = kt * NB_T;
        __syncthreads();   // every wave has finished reading the previous tile
        if constexpr (PREF) {
            kregs.store((uint16_t*)Ks, tid);
            vregs.store((uint16_t*)Vs, tid);
            ktregs.store((uint16_t*)Kt, tid);
        } else {
            nb_stage_rows<DT, D, Cfg::STR>(Ks, kbase, p.ldk, key0, p.Lk, tid);
            nb_stage_rows<DT, D, Cfg::STR>(Vs, vbase, p.ldv, key0, p.Lk, tid);
            if constexpr (DT == DAT_BF16) nb_stage_tr<DV>(Kt, kbase + dv0, p.ldk, key0, p.Lk, tid);
        }
        __syncthreads();
        if constexpr (PREF)
            if (kt + 1 < ntiles) load_tile(key0 + NB_T);
        if (!wave_active) continue;

        // S^T = K Q^T and dP^T = V dY^T: row = key (accumulator register), column = query (lane & 31)
        const f32x16_t sacc = nb_row_product<DT, D, Cfg::STR, Cfg::NQ, Cfg::REG>(Ks, qf, qp, qvalid, r, h);
        const f32x16_t dpacc = nb_row_product<DT, D, Cfg::STR, Cfg::NQ, Cfg::REG>(Vs, dyf, dyp, qvalid, r, h);
        float ds[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float pv = key0 + nb_crow(i, h) < p.Lk ? __builtin_amdgcn_exp2f(sacc[i] * p.c - lse_i) : 0.f;
            ds[i] = pv * (dpacc[i] - del_i);
        }
        // dQ^T += K^T dS^T: row = channel, column = query
        nb_col_product<DT, DV, Cfg::STR>(acc, Kt, Ks, dv0, ds, r, h);
    }

    if (!qvalid) return;
    nb_store<DT, DV>((T*)p.dq + (size_t)(clip * p.Lq + qrow) * p.lddq + dv0, acc, p.scale, h);
}

template <int DT, int D, int DV>
__global__ __launch_bounds__(256) void nl_bwd_dkdv_kernel(NbParams p) {
    typedef NbCfg<DT, D, DV> Cfg;
    typedef typename ElemOf<DT>::type T;
    extern __shared__ __align__(16) unsigned char nb_smem[];
    T* Qs = (T*)nb_smem;
    T* Ys = (T*)(nb_smem + Cfg::ROW_BYTES);
    T* Qt = (T*)(nb_smem + 2 * Cfg::ROW_BYTES);
    T* Yt = (T*)(nb_smem + 2 * Cfg::ROW_BYTES + Cfg::TR_BYTES);
    float* lse_s = (float*)(nb_smem + 2 * Cfg::ROW_BYTES + 2 * Cfg::TR_BYTES);
    float* del_s = lse_s + NB_T;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const long long clip = blockIdx.y;
    const long long k0 = (long long)blockIdx.x * NB_ROWS + wave * 32;
    const int dv0 = (int)blockIdx.z * DV;
    const long long krow = k0 + r;
    const bool kvalid = krow < p.Lk;
    const bool wave_active = k0 < p.Lk;

    const T* qbase = (const T*)p.q + (size_t)(clip * p.Lq) * p.ldq;
    const T* dybase = (const T*)p.dy + (size_t)(clip * p.Lq) * p.lddy;
    const float* lse = p.lse + clip * p.Lq;
    const float* delta = p.delta + clip * p.Lq;
    const size_t grow = (size_t)(clip * p.Lk + (kvalid ? krow : 0));
    const T* kp = (const T*)p.k + grow * p.ldk;
    const T* vp = (const T*)p.v + grow * p.ldv;

    uint32_t kf[Cfg::REG ? Cfg::NQ : 1], vf[Cfg::REG ? Cfg::NQ : 1];
    if constexpr (Cfg::REG) {
        nb_load_frag<DT, D, Cfg::NQ>(kf, kp, kvalid, h);
        nb_load_frag<DT, D, Cfg::NQ>(vf, vp, kvalid, h);
    }

    f32x16_t dkacc[DV / 32], dvacc[DV / 32];
#pragma unroll
    for (int n = 0; n < DV / 32; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) dkacc[n][i] = dvacc[n][i] = 0.f;

    constexpr bool PREF = Cfg::PREF;
    NbRowRegs<PREF ? D : 64, Cfg::STR> qregs, yregs;
    NbTrRegs<PREF ? DV : 64> qtregs, ytregs;
    float stat = 0.f;   // threads 0 .. 31: lse of the tile's row, threads 32 .. 63: delta
    auto load_tile = [&](long long row0) {
        qregs.load((const uint16_t*)qbase, p.ldq, row0, p.Lq, tid);
        yregs.load((const uint16_t*)dybase, p.lddy, row0, p.Lq, tid);
        qtregs.load((const uint16_t*)qbase + dv0, p.ldq, row0, p.Lq, tid);
        ytregs.load((const uint16_t*)dybase + dv0, p.lddy, row0, p.Lq, tid);
        stat = 0.f;
        if (tid < NB_T) { if (row0 + tid < p.Lq) stat = lse[row0 + tid]; }
        else if (tid < 2 * NB_T) { if (row0 + tid - NB_T < p.Lq) stat = delta[row0 + tid - NB_T]; }
    };
    const long long ntiles = (p.Lq + NB_T - 1) / NB_T;
    if constexpr (PREF) load_tile(0);
    for (long long qt = 0; qt < ntiles; ++qt) {
        const long long row0 = qt * NB_T;
        __syncthreads();
        if constexpr (PREF) {
            qregs.store((uint16_t*)Qs, tid);
            yregs.store((uint16_t*)Ys, tid);
            qtregs.store((uint16_t*)Qt, tid);
            ytregs.store((uint16_t*)Yt, tid);
            if (tid < 2 * NB_T) lse_s[tid] = stat;   // (del_s follows lse_s)
        } else {
            nb_stage_rows<DT, D, Cfg::STR>(Qs, qbase, p.ldq, row0, p.Lq, tid);
            nb_stage_rows<DT, D, Cfg::STR>(Ys, dybase, p.lddy, row0, p.Lq, tid);
            if constexpr (DT == DAT_BF16) {
                nb_stage_tr<DV>(Qt, qbase + dv0, p.ldq, row0, p.Lq, tid);
                nb_stage_tr<DV>(Yt, dybase + dv0, p.lddy, row0, p.Lq, tid);
            }
            if (tid < NB_T) lse_s[tid] = row0 + tid < p.Lq ? lse[row0 + tid] : 0.f;
            else if (tid < 2 * NB_T) del_s[tid - NB_T] = row0 + tid - NB_T < p.Lq ? delta[row0 + tid - NB_T] : 0.f;
        }
        __syncthreads();
        if constexpr (PREF)
            if (qt + 1 < ntiles) load_tile(row0 + NB_T);
        if (!wave_active) continue;

        // S = Q K^T and dP = dY V^T: row = query (accumulator register), column = key (lane & 31)
        const f32x16_t sacc = nb_row_product<DT, D, Cfg::STR, Cfg::NQ, Cfg::REG>(Qs, kf, kp, kvalid, r, h);
        const f32x16_t dpacc = nb_row_product<DT, D, Cfg::STR, Cfg::NQ, Cfg::REG>(Ys, vf, vp, kvalid, r, h);
        float pv[16], ds[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int qi = nb_crow(i, h);
            pv[i] = (kvalid && row0 + qi < p.Lq) ? __builtin_amdgcn_exp2f(sacc[i] * p.c - lse_s[qi]) : 0.f;
            ds[i] = pv[i] * (dpacc[i] - del_s[qi]);
        }
        // dV^T += dY^T P and dK^T += Q^T dS: row = channel, column = key
        nb_col_product<DT, DV, Cfg::STR>(dvacc, Yt, Ys, dv0, pv, r, h);
        nb_col_product<DT, DV, Cfg::STR>(dkacc, Qt, Qs, dv0, ds, r, h);
    }

    if (!kvalid) return;
    nb_store<DT, DV>((T*)p.dk + (size_t)(clip * p.Lk + krow) * p.lddk + dv0, dkacc, p.scale, h);
    nb_store<DT, DV>((T*)p.dv + (size_t)(clip * p.Lk + krow) * p.lddv + dv0, dvacc, 1.f, h);
}

template <int DT, int D, int DVQ, int DVK>
int nb_launch(dat_ctx* ctx, hipStream_t s, const dat_nonlocal_bwd_desc* d, const NbParams& p) {
    const void* kq = (const void*)nl_bwd_dq_kernel<DT, D, DVQ>;
    const void* kk = (const void*)nl_bwd_dkdv_kernel<DT, D, DVK>;
    constexpr int lds_q = NbCfg<DT, D, DVQ>::DQ_LDS, lds_k = NbCfg<DT, D, DVK>::DKDV_LDS;
    int rc = dat_ensure_lds(ctx, kq, lds_q);
    if (rc != DAT_OK) return rc;
    rc = dat_ensure_lds(ctx, kk, lds_k);
    if (rc != DAT_OK) return rc;
    const dim3 gq((unsigned)((d->Lq + NB_ROWS - 1) / NB_ROWS), (unsigned)d->clips, (unsigned)(D / DVQ));
    hipLaunchKernelGGL((nl_bwd_dq_kernel<DT, D, DVQ>), gq, dim3(256), lds_q, s, p);
    DAT_CHECK_LAUNCH(ctx, "nonlocal_attention_bwd (dq)");
    const dim3 gk((unsigned)((d->Lk + NB_ROWS - 1) / NB_ROWS), (unsigned)d->clips, (unsigned)(D / DVK));
    hipLaunchKernelGGL((nl_bwd_dkdv_kernel<DT, D, DVK>), gk, dim3(256), lds_k, s, p);
    DAT_CHECK_LAUNCH(ctx, "nonlocal_attention_bwd (dk, dv)");
    return DAT_OK;
}

// ---- max-pool backward, non-overlapping windows (k <= stride): every input element belongs to at most one window
template <int DT>
__global__ void maxpool_hw_bwd_kernel(const void* __restrict__ x, const void* __restrict__ dy, void* __restrict__ dx, int frames, int H, int W,
                                      int C, int Ho, int Wo, int k, int stride, int pad) {
    typedef typename ElemOf<DT>::type T;
    constexpr int V = 16 / ElemOf<DT>::size;
    const int cv = C / V;
    const size_t total = (size_t)frames * H * W * cv;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int cg = i % cv;
        size_t t = i / cv;
        const int w = t % W; t /= W;
        const int hh = t % H;
        const int f = t / H;
        const int oh = (hh + pad) / stride, ow = (w + pad) / stride;
        __align__(16) T out[V];
#pragma unroll
        for (int j = 0; j < V; ++j) out[j] = 0;
        if (oh < Ho && ow < Wo && hh + pad - oh * stride < k && w + pad - ow * stride < k) {
            // the first maximum of the window in (h, w) scan order takes the gradient (torch's max_pool2d on the host)
            float best[V];
            bool mine[V];
#pragma unroll
            for (int j = 0; j < V; ++j) { best[j] = -INFINITY; mine[j] = false; }
            for (int kh = 0; kh < k; ++kh) {
                const int ih = oh * stride - pad + kh;
                if (ih < 0 || ih >= H) continue;
                for (int kw = 0; kw < k; ++kw) {
                    const int iw = ow * stride - pad + kw;
                    if (iw < 0 || iw >= W) continue;
                    __align__(16) T v[V];
                    *(u32x4_t*)v = *(const u32x4_t*)((const T*)x + (((size_t)f * H + ih) * W + iw) * C + cg * V);
                    const bool me = ih == hh && iw == w;
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        float fv;
                        if constexpr (DT == DAT_BF16) fv = bf2f(v[j]); else fv = v[j];
                        if (fv > best[j]) { best[j] = fv; mine[j] = me; }
                    }
                }
            }
            __align__(16) T g[V];
            *(u32x4_t*)g = *(const u32x4_t*)((const T*)dy + (((size_t)f * Ho + oh) * Wo + ow) * C + cg * V);
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (mine[j]) out[j] = g[j];
        }
        *(u32x4_t*)((T*)dx + i * V) = *(const u32x4_t*)out;
    }
}

}  // namespace

extern "C" {

int dat_nonlocal_attention_bwd(dat_ctx* ctx, dat_stream s, const dat_nonlocal_bwd_desc* d, const void* q, const void* k, const void* v,
                               const void* y, const void* dy, const float* lse, float* delta, void* dq, void* dk, void* dv) {
    DAT_ENFORCE(ctx, ctx && d, "nonlocal_attention_bwd: null context or descriptor");
    if (d->dtype != DAT_F32 && d->dtype != DAT_BF16)
        DAT_FAIL(ctx, DAT_ERR_UNSUPPORTED, "nonlocal_attention_bwd: dtype %d (DAT_F32 | DAT_BF16)", d->dtype);
    if (d->D != 64 && d->D != 128 && d->D != 256 && d->D != 512)
        DAT_FAIL(ctx, DAT_ERR_UNSUPPORTED, "nonlocal_attention_bwd: D = %d channels (64 | 128 | 256 | 512)", d->D);
    DAT_ENFORCE(ctx, d->clips >= 1 && d->clips <= 65535, "nonlocal_attention_bwd: %d clips (1 .. 65535)", d->clips);
    DAT_ENFORCE(ctx, d->Lq >= 1 && d->Lk >= 1, "nonlocal_attention_bwd: Lq = %lld, Lk = %lld rows per clip (>= 1 each)", d->Lq, d->Lk);
    DAT_ENFORCE(ctx, d->Lq <= (1ll << 37) && d->Lk <= (1ll << 37) && d->clips * d->Lq <= (1ll << 40) && d->clips * d->Lk <= (1ll << 40),
                "nonlocal_attention_bwd: %d clips of Lq = %lld, Lk = %lld rows", d->clips, d->Lq, d->Lk);
    const int lds[8] = {d->ldq, d->ldk, d->ldv, d->ldy, d->lddy, d->lddq, d->lddk, d->lddv};
    const char* const names[8] = {"ldq", "ldk", "ldv", "ldy", "lddy", "lddq", "lddk", "lddv"};
    for (int i = 0; i < 8; ++i)
        DAT_ENFORCE(ctx, lds[i] >= d->D && lds[i] % 8 == 0, "nonlocal_attention_bwd: %s = %d (>= D = %d and a multiple of 8)", names[i],
                    lds[i], d->D);
    DAT_ENFORCE(ctx, d->scale == d->scale && d->scale - d->scale == 0.f, "nonlocal_attention_bwd: scale is not finite");
    DAT_ENFORCE(ctx, q && k && v && y && dy && lse && delta && dq && dk && dv,
                "nonlocal_attention_bwd: null pointer (q %p, k %p, v %p, y %p, dy %p, lse %p, delta %p, dq %p, dk %p, dv %p)", q, k, v, y, dy,
                (const void*)lse, (void*)delta, dq, dk, dv);
    DAT_ENFORCE(ctx, (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)y | (uintptr_t)dy | (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv) & 15) == 0,
                "nonlocal_attention_bwd: q, k, v, y, dy, dq, dk and dv must be 16-byte aligned");
    DAT_ENFORCE(ctx, (((uintptr_t)lse | (uintptr_t)delta) & 3) == 0, "nonlocal_attention_bwd: lse and delta must be 4-byte aligned");
    hipStream_t st = (hipStream_t)s;
    const long long rows = d->clips * d->Lq;
    const unsigned dgrid = (unsigned)((rows * 16 + 255) / 256);
    if (d->dtype == DAT_BF16)
        hipLaunchKernelGGL((nl_delta_kernel<DAT_BF16>), dim3(dgrid), dim3(256), 0, st, y, dy, delta, rows, d->D, d->ldy, d->lddy);
    else
        hipLaunchKernelGGL((nl_delta_kernel<DAT_F32>), dim3(dgrid), dim3(256), 0, st, y, dy, delta, rows, d->D, d->ldy, d->lddy);
    DAT_CHECK_LAUNCH(ctx, "nonlocal_attention_bwd (delta)");
    NbParams p;
    p.q = q; p.k = k; p.v = v; p.dy = dy;
    p.lse = lse; p.delta = delta;
    p.dq = dq; p.dk = dk; p.dv = dv;
    p.Lq = d->Lq; p.Lk = d->Lk;
    p.ldq = d->ldq; p.ldk = d->ldk; p.ldv = d->ldv; p.lddy = d->lddy; p.lddq = d->lddq; p.lddk = d->lddk; p.lddv = d->lddv;
    p.c = d->scale * 1.44269504088896340736f;
    p.scale = d->scale;
    // <dtype, D, channels of a dq slice, channels of a dk / dv slice>
    if (d->dtype == DAT_BF16) {
        switch (d->D) {
            case 64: return nb_launch<DAT_BF16, 64, 64, 64>(ctx, st, d, p);
            case 128: return nb_launch<DAT_BF16, 128, 128, 128>(ctx, st, d, p);
            case 256: return nb_launch<DAT_BF16, 256, 256, 128>(ctx, st, d, p);
            default: return nb_launch<DAT_BF16, 512, 128, 64>(ctx, st, d, p);
        }
    }
    switch (d->D) {
        case 64: return nb_launch<DAT_F32, 64, 64, 64>(ctx, st, d, p);
        case 128: return nb_launch<DAT_F32, 128, 128, 64>(ctx, st, d, p);
        case 256: return nb_launch<DAT_F32, 256, 64, 64>(ctx, st, d, p);
        default: return nb_launch<DAT_F32, 512, 64, 64>(ctx, st, d, p);
    }
}

int dat_maxpool_hw_bwd(dat_ctx* ctx, dat_stream s, int dtype, const void* x, const void* dy, void* dx, int frames, int H, int W, int C, int k,
                       int stride, int pad) {
    DAT_ENFORCE(ctx, ctx, "maxpool_hw_bwd: null context");
    if (dtype != DAT_F32 && dtype != DAT_BF16) DAT_FAIL(ctx, DAT_ERR_UNSUPPORTED, "maxpool_hw_bwd: dtype %d (DAT_F32 | DAT_BF16)", dtype);
    DAT_ENFORCE(ctx, x && dy && dx, "maxpool_hw_bwd: null pointer (x %p, dy %p, dx %p)", x, dy, dx);
    DAT_ENFORCE(ctx, (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 15) == 0, "maxpool_hw_bwd: x, dy and dx must be 16-byte aligned");
    DAT_ENFORCE(ctx, C >= 8 && C % 8 == 0, "maxpool_hw_bwd: C = %d must be a positive multiple of 8", C);
    DAT_ENFORCE(ctx, frames >= 1 && H >= 1 && W >= 1, "maxpool_hw_bwd: %d frames of %d x %d", frames, H, W);
    DAT_ENFORCE(ctx, k >= 1 && k <= stride, "maxpool_hw_bwd: kernel %d, stride %d: windows must not overlap (1 <= k <= stride)", k, stride);
    DAT_ENFORCE(ctx, pad >= 0 && pad < k, "maxpool_hw_bwd: pad %d (0 <= pad < k = %d)", pad, k);
    DAT_ENFORCE(ctx, H + 2 * pad >= k && W + 2 * pad >= k, "maxpool_hw_bwd: a %d x %d map holds no %d x %d window", H, W, k, k);
    const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    const size_t total = (size_t)frames * H * W * (C / (16 / dat_esize(dtype)));
    const size_t blocks = (total + 255) / 256;
    const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536));
    if (dtype == DAT_BF16)
        hipLaunchKernelGGL((maxpool_hw_bwd_kernel<DAT_BF16>), grid, dim3(256), 0, (hipStream_t)s, x, dy, dx, frames, H, W, C, Ho, Wo, k, stride, pad);
    else
        hipLaunchKernelGGL((maxpool_hw_bwd_kernel<DAT_F32>), grid, dim3(256), 0, (hipStream_t)s, x, dy, dx, frames, H, W, C, Ho, Wo, k, stride, pad);
    DAT_CHECK_LAUNCH(ctx, "maxpool_hw_bwd");
    return DAT_OK;
}

}  // extern "C"
