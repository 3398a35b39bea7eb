// Spacetime non-local block (HIP.NONLOCAL): y = softmax(scale * q k^T) v per clip, fused -- the
// [Lq, Lk] score matrix never reaches memory (one res4 block of the benched clip would be 1 GB, one res3 block 16.6 GB).
//
// A workgroup is four waves, each owning 32 query rows whose q fragments stay in registers for the whole key loop.  Keys and
// values arrive in tiles of 32 rows, staged in LDS once per workgroup.  Per tile a wave computes the SWAPPED product
// S^T = K Q^T, so a lane holds 16 of the 32 scores of ONE query row (the other 16 sit in lane ^ 32): the row maximum and the
// row sum are in-lane plus one lane exchange.  O^T = V^T P^T then takes the P tile straight from the score accumulator as its
// B operand (the k order inside an MFMA step is permuted: element j of lane half h is key 16 s + 8 (j >> 2) + 4 h + (j & 3),
// and the V^T fragment is read from LDS in that same order), and its result again has the query on the lane, so the online
// rescale of O is a per-lane multiply.
// For D <= 256 in 16 bits the global loads of the next tile are issued before the MFMAs of the current one and wait in registers.
//
// Numerics: scores accumulate in fp32; scale * log2(e) is one fp32 constant applied to the accumulated score; the running
// row maximum is subtracted; keys >= Lk get -inf (a zero-filled LDS row is not an excluded key: it would score exp(-max));
// the denominator sums the UNROUNDED p in fp32; on the 16-bit path p is rounded to nearest once for the PV MFMA; the output is
// divided by the denominator and rounded once.  DAT_F32 runs both products on v_mfma_f32_32x32x2_f32 (exact fp32 fma chains).
//
// No workspace, no atomics, no host synchronisation; the key loop is sequential per query row, so the result is bitwise
// reproducible and does not depend on the number of clips in the launch.
#include "dat_common.h"

#include <type_traits>

namespace {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2_t;

constexpr int NL_ROWS = 128;   // query rows per workgroup (4 waves x 32)
constexpr int NL_KT = 32;      // keys per tile

struct NlParams {
    const void *q, *k, *v;
    void* y;
    long long Lq, Lk;
    int ldq, ldk, ldv, ldy;
    float c;   // scale * log2(e)
};
// the training forward also stores the row statistic lse_i = m_i + log2(l_i) (in the units of c * score) that the backward recomputes P from
struct NlParamsLse : NlParams {
    float* lse;
};

template <int DT, int D, int DV>
struct NlCfg {
    static constexpr int ES = DT == DAT_BF16 ? 2 : 4;
    // K tile [32 keys][KSTR]: 16-bit rows padded by 16 bytes (b128 fragment reads of 32 rows), fp32 rows by 2 floats (lane (r, h) reads
    // bank 2 r + h)
    static constexpr int KSTR = DT == DAT_BF16 ? D + 8 : D + 2;
    // 16-bit: V TRANSPOSED, [DV channels][36] (32 keys + 8 bytes of padding); fp32: [32 keys][DV + 8]
    static constexpr int VSTR = DT == DAT_BF16 ? 36 : DV + 8;
    static constexpr int K_BYTES = NL_KT * KSTR * ES;
    static constexpr int V_BYTES = DT == DAT_BF16 ? DV * VSTR * 2 : NL_KT * VSTR * 4;
    static constexpr int LDS_BYTES = K_BYTES + V_BYTES;
    static constexpr int NQ = DT == DAT_BF16 ? D / 16 * 4 : D / 2;   // registers of a lane's q fragments
};

// row of a 32 x 32 MFMA result held in accumulator register `reg` of lane half `h`
__device__ __forceinline__ int nl_crow(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

template <int DT, int D, int DV, bool LSE>
__global__ __launch_bounds__(256) void nonlocal_attention_kernel(typename std::conditional<LSE, NlParamsLse, NlParams>::type p) {
    typedef NlCfg<DT, D, DV> Cfg;
    typedef typename ElemOf<DT>::type T;
    extern __shared__ __align__(16) unsigned char nl_smem[];
    T* Ks = (T*)nl_smem;
    T* Vs = (T*)(nl_smem + Cfg::K_BYTES);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const long long clip = blockIdx.y;
    const long long q0 = (long long)blockIdx.x * NL_ROWS + wave * 32;
    const int dv0 = (int)blockIdx.z * DV;
    const long long qrow = q0 + r;
    const bool qvalid = qrow < p.Lq;
    const bool wave_active = q0 < p.Lq;   // wave-uniform: a wave past the last row still stages tiles and meets the barriers

    const T* kbase = (const T*)p.k + (size_t)(clip * p.Lk) * p.ldk;
    const T* vbase = (const T*)p.v + (size_t)(clip * p.Lk) * p.ldv + dv0;

    // ---- this lane's q fragments: the B operand of every score MFMA
    uint32_t qf[Cfg::NQ];
    {
        const T* qp = (const T*)p.q + (size_t)(clip * p.Lq + (qvalid ? qrow : 0)) * p.ldq;
        if constexpr (DT == DAT_BF16) {
#pragma unroll
            for (int s = 0; s < D / 16; ++s) {
                u32x4_t t = {0u, 0u, 0u, 0u};
                if (qvalid) t = *(const u32x4_t*)(qp + 16 * s + 8 * h);
                qf[4 * s] = t.x; qf[4 * s + 1] = t.y; qf[4 * s + 2] = t.z; qf[4 * s + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int s = 0; s < D / 2; ++s)   // k step s takes channel 2 s + h (dword loads: vector loads would hold 2 D registers at once)
                qf[s] = qvalid ? ((const uint32_t*)qp)[2 * s + h] : 0u;
        }
    }

    f32x16_t oacc[DV / 32];
#pragma unroll
    for (int n = 0; n < DV / 32; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[n][i] = 0.f;
    float m_run = -INFINITY;   // running maximum of c * score (both lane halves agree)
    float l_run = 0.f;         // this lane half's part of the denominator

    // 16-bit path: a thread's share of a K / V tile on its way from HBM to LDS.  With PREF the loads of tile kt + 1 are issued before the
    // MFMAs of tile kt and stay in flight under them (D = 512 has no registers left for that: its tiles go from HBM to LDS chunk by chunk)
    constexpr bool PREF = DT == DAT_BF16 && D <= 256;
    constexpr int NKC = PREF ? D / 64 : 1;                 // 16-byte K chunks per thread: 32 * (D / 8) / 256
    constexpr int NVC = PREF ? (DV + 127) / 128 : 1;       // V items (two adjacent keys x 8 channels) per thread: 16 * (DV / 8) / 256
    u32x4_t kreg[NKC], vra[NVC], vrb[NVC];
    auto load_tile = [&](long long key0) {
#pragma unroll
        for (int i = 0; i < NKC; ++i) {
            const int c = tid + i * 256, row = c / (D / 8), c8 = c % (D / 8);
            kreg[i] = u32x4_t{0u, 0u, 0u, 0u};
            if (key0 + row < p.Lk) kreg[i] = *(const u32x4_t*)(kbase + (size_t)(key0 + row) * p.ldk + c8 * 8);
        }
#pragma unroll
        for (int i = 0; i < NVC; ++i) {
            const int c = tid + i * 256, kp = c / (DV / 8), c8 = c % (DV / 8);
            vra[i] = vrb[i] = u32x4_t{0u, 0u, 0u, 0u};
            if (c < (NL_KT / 2) * (DV / 8)) {
                if (key0 + 2 * kp < p.Lk) vra[i] = *(const u32x4_t*)(vbase + (size_t)(key0 + 2 * kp) * p.ldv + c8 * 8);
                if (key0 + 2 * kp + 1 < p.Lk) vrb[i] = *(const u32x4_t*)(vbase + (size_t)(key0 + 2 * kp + 1) * p.ldv + c8 * 8);
            }
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < NKC; ++i) {
            const int c = tid + i * 256, row = c / (D / 8), c8 = c % (D / 8);
            *(u32x4_t*)(Ks + row * Cfg::KSTR + c8 * 8) = kreg[i];
        }
        // V transposed: one item = two adjacent keys x 8 channels -> 8 dword stores Vt[channel][key pair]
#pragma unroll
        for (int i = 0; i < NVC; ++i) {
            const int c = tid + i * 256, kp = c / (DV / 8), c8 = c % (DV / 8);
            if (c < (NL_KT / 2) * (DV / 8)) {
                uint32_t* dst = (uint32_t*)(Vs + (c8 * 8) * Cfg::VSTR + 2 * kp);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t wa = vra[i][j], wb = vrb[i][j];
                    dst[(2 * j) * (Cfg::VSTR / 2)] = (wa & 0xffffu) | (wb << 16);
                    dst[(2 * j + 1) * (Cfg::VSTR / 2)] = (wa >> 16) | (wb & 0xffff0000u);
                }
            }
        }
    };

    const long long ntiles = (p.Lk + NL_KT - 1) / NL_KT;
    if constexpr (PREF) load_tile(0);
    for (long long kt = 0; kt < ntiles; ++kt) {
        const long long key0 = kt * NL_KT;
        __syncthreads();   // every wave has finished reading the previous tile
        // ---- stage K [32][D] and V [32][DV]; rows at or past Lk are zero-filled (and masked below)
        if constexpr (DT == DAT_BF16) {
            if constexpr (PREF) {
                store_tile();
            } else {
                for (int c = tid; c < NL_KT * (D / 8); c += 256) {
                    const int row = c / (D / 8), c8 = c % (D / 8);
                    u32x4_t t = {0u, 0u, 0u, 0u};
                    if (key0 + row < p.Lk) t = *(const u32x4_t*)(kbase + (size_t)(key0 + row) * p.ldk + c8 * 8);
                    *(u32x4_t*)(Ks + row * Cfg::KSTR + c8 * 8) = t;
                }
                // V transposed: one item = two adjacent keys x 8 channels -> 8 dword stores Vt[channel][key pair]
                for (int c = tid; c < (NL_KT / 2) * (DV / 8); c += 256) {
                    const int kp = c / (DV / 8), c8 = c % (DV / 8);
                    u32x4_t a = {0u, 0u, 0u, 0u}, b = {0u, 0u, 0u, 0u};
                    if (key0 + 2 * kp < p.Lk) a = *(const u32x4_t*)(vbase + (size_t)(key0 + 2 * kp) * p.ldv + c8 * 8);
                    if (key0 + 2 * kp + 1 < p.Lk) b = *(const u32x4_t*)(vbase + (size_t)(key0 + 2 * kp + 1) * p.ldv + c8 * 8);
                    uint32_t* dst = (uint32_t*)(Vs + (c8 * 8) * Cfg::VSTR + 2 * kp);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const uint32_t wa = a[i], wb = b[i];
                        dst[(2 * i) * (Cfg::VSTR / 2)] = (wa & 0xffffu) | (wb << 16);
                        dst[(2 * i + 1) * (Cfg::VSTR / 2)] = (wa >> 16) | (wb & 0xffff0000u);
                    }
                }
            }
        } else {
            for (int c = tid; c < NL_KT * (D / 4); c += 256) {
                const int row = c / (D / 4), c4 = c % (D / 4);
                u32x4_t t = {0u, 0u, 0u, 0u};
                if (key0 + row < p.Lk) t = *(const u32x4_t*)(kbase + (size_t)(key0 + row) * p.ldk + c4 * 4);
                u32x2_t* dst = (u32x2_t*)(Ks + row * Cfg::KSTR + c4 * 4);   // rows are 8-byte aligned only
                dst[0] = u32x2_t{t.x, t.y};
                dst[1] = u32x2_t{t.z, t.w};
            }
            for (int c = tid; c < NL_KT * (DV / 4); c += 256) {
                const int row = c / (DV / 4), c4 = c % (DV / 4);
                u32x4_t t = {0u, 0u, 0u, 0u};
                if (key0 + row < p.Lk) t = *(const u32x4_t*)(vbase + (size_t)(key0 + row) * p.ldv + c4 * 4);
                *(u32x4_t*)(Vs + row * Cfg::VSTR + c4 * 4) = t;
            }
        }
        __syncthreads();
        if constexpr (PREF)
            if (kt + 1 < ntiles) load_tile(key0 + NL_KT);
        if (!wave_active) continue;

        // ---- S^T = K Q^T: row = key (accumulator register), column = query (lane & 31)
        f32x16_t sacc;
#pragma unroll
        for (int i = 0; i < 16; ++i) sacc[i] = 0.f;
        if constexpr (DT == DAT_BF16) {
#pragma unroll
            for (int s = 0; s < D / 16; ++s) {
                const u32x4_t a = *(const u32x4_t*)(Ks + r * Cfg::KSTR + 16 * s + 8 * h);
                const u32x4_t b = {qf[4 * s], qf[4 * s + 1], qf[4 * s + 2], qf[4 * s + 3]};
                sacc = DAT_MFMA16(a, b, sacc);
            }
        } else {
#pragma unroll
            for (int s = 0; s < D / 2; ++s) {
                sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[r * Cfg::KSTR + 2 * s + h], __uint_as_float(qf[s]), sacc, 0, 0, 0);
            }
        }

        // ---- online softmax of this query row
        float t[16];
        float mt = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            t[i] = key0 + nl_crow(i, h) < p.Lk ? sacc[i] * p.c : -INFINITY;
            mt = fmaxf(mt, t[i]);
        }
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float m_new = fmaxf(m_run, mt);   // finite: key0 < Lk, so every tile holds a valid key
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        m_run = m_new;
        float ps = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            t[i] = __builtin_amdgcn_exp2f(t[i] - m_new);
            ps += t[i];
        }
        l_run = l_run * alpha + ps;
#pragma unroll
        for (int n = 0; n < DV / 32; ++n)
#pragma unroll
            for (int i = 0; i < 16; ++i) oacc[n][i] *= alpha;

        // ---- O^T += V^T P^T: row = value channel, column = query
        if constexpr (DT == DAT_BF16) {
            u32x4_t pb[2];
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int i = 0; i < 4; ++i) pb[s][i] = f2bf2(t[8 * s + 2 * i], t[8 * s + 2 * i + 1]);   // round to nearest even
#pragma unroll
            for (int n = 0; n < DV / 32; ++n) {
                const T* vrow = Vs + (n * 32 + r) * Cfg::VSTR;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const u32x2_t lo = *(const u32x2_t*)(vrow + 16 * s + 4 * h);
                    const u32x2_t hi = *(const u32x2_t*)(vrow + 16 * s + 8 + 4 * h);
                    const u32x4_t a = {lo.x, lo.y, hi.x, hi.y};
                    oacc[n] = DAT_MFMA16(a, pb[s], oacc[n]);
                }
            }
        } else {
#pragma unroll
            for (int n = 0; n < DV / 32; ++n)
#pragma unroll
                for (int i = 0; i < 16; ++i)   // k step i: lane half h supplies key crow(i, h), the key whose p it holds in register i
                    oacc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[nl_crow(i, h) * Cfg::VSTR + n * 32 + r], t[i], oacc[n], 0, 0, 0);
        }
    }

    if (!qvalid) return;
    const float l = l_run + __shfl_xor(l_run, 32);   // the partner lane holds the same (valid) query row
    if constexpr (LSE)
        if (h == 0 && blockIdx.z == 0) p.lse[clip * p.Lq + qrow] = m_run + __log2f(l);
    T* yp = (T*)p.y + (size_t)(clip * p.Lq + qrow) * p.ldy + dv0;
#pragma unroll
    for (int n = 0; n < DV / 32; ++n)
#pragma unroll
        for (int g = 0; g < 4; ++g) {   // registers 4 g .. 4 g + 3: channels n * 32 + 8 g + 4 h + (0 .. 3)
            const float o0 = oacc[n][4 * g] / l, o1 = oacc[n][4 * g + 1] / l, o2 = oacc[n][4 * g + 2] / l, o3 = oacc[n][4 * g + 3] / l;
            T* dst = yp + n * 32 + 8 * g + 4 * h;
            if constexpr (DT == DAT_BF16)
                *(u32x2_t*)dst = u32x2_t{f2bf2(o0, o1), f2bf2(o2, o3)};
            else
                *(f32x4_t*)dst = f32x4_t{o0, o1, o2, o3};
        }
}

template <int DT, int D, int DV, bool LSE>
int nl_launch(dat_ctx* ctx, hipStream_t s, const dat_nonlocal_desc* d, const typename std::conditional<LSE, NlParamsLse, NlParams>::type& p) {
    typedef NlCfg<DT, D, DV> Cfg;
    const void* kern = (const void*)nonlocal_attention_kernel<DT, D, DV, LSE>;
    const int rc = dat_ensure_lds(ctx, kern, Cfg::LDS_BYTES);
    if (rc != DAT_OK) return rc;
    const dim3 grid((unsigned)((d->Lq + NL_ROWS - 1) / NL_ROWS), (unsigned)d->clips, (unsigned)(D / DV));
    hipLaunchKernelGGL((nonlocal_attention_kernel<DT, D, DV, LSE>), grid, dim3(256), Cfg::LDS_BYTES, s, p);
    DAT_CHECK_LAUNCH(ctx, "nonlocal_attention");
    return DAT_OK;
}

// argument checks shared by the two forward entry points; fills the launch parameters
int nl_check(dat_ctx* ctx, const dat_nonlocal_desc* d, const void* q, const void* k, const void* v, void* y, NlParams& p) {
    DAT_ENFORCE(ctx, ctx && d, "nonlocal_attention: null context or descriptor");
    if (d->dtype != DAT_F32 && d->dtype != DAT_BF16)
        DAT_FAIL(ctx, DAT_ERR_UNSUPPORTED, "nonlocal_attention: dtype %d (DAT_F32 | DAT_BF16)", d->dtype);
    if (d->D != 64 && d->D != 128 && d->D != 256 && d->D != 512)
        DAT_FAIL(ctx, DAT_ERR_UNSUPPORTED, "nonlocal_attention: D = %d channels (64 | 128 | 256 | 512)", d->D);
    DAT_ENFORCE(ctx, d->clips >= 1 && d->clips <= 65535, "nonlocal_attention: %d clips (1 .. 65535)", d->clips);
    DAT_ENFORCE(ctx, d->Lq >= 1 && d->Lk >= 1, "nonlocal_attention: Lq = %lld, Lk = %lld rows per clip (>= 1 each)", d->Lq, d->Lk);
    DAT_ENFORCE(ctx, d->Lq <= (1ll << 37) && d->Lk <= (1ll << 37) && d->clips * d->Lq <= (1ll << 40) && d->clips * d->Lk <= (1ll << 40),
                "nonlocal_attention: %d clips of Lq = %lld, Lk = %lld rows", d->clips, d->Lq, d->Lk);
    const int lds[4] = {d->ldq, d->ldk, d->ldv, d->ldy};
    const char* const names[4] = {"ldq", "ldk", "ldv", "ldy"};
    for (int i = 0; i < 4; ++i)
        DAT_ENFORCE(ctx, lds[i] >= d->D && lds[i] % 8 == 0, "nonlocal_attention: %s = %d (>= D = %d and a multiple of 8)", names[i], lds[i],
                    d->D);
    DAT_ENFORCE(ctx, d->scale == d->scale && d->scale - d->scale == 0.f, "nonlocal_attention: scale is not finite");
    DAT_ENFORCE(ctx, q && k && v && y, "nonlocal_attention: null pointer (q %p, k %p, v %p, y %p)", q, k, v, y);
    DAT_ENFORCE(ctx, (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)y) & 15) == 0,
                "nonlocal_attention: q, k, v and y must be 16-byte aligned");
    p.q = q; p.k = k; p.v = v; p.y = y;
    p.Lq = d->Lq; p.Lk = d->Lk;
    p.ldq = d->ldq; p.ldk = d->ldk; p.ldv = d->ldv; p.ldy = d->ldy;
    p.c = d->scale * 1.44269504088896340736f;
    return DAT_OK;
}

template <bool LSE>
int nl_dispatch(dat_ctx* ctx, hipStream_t st, const dat_nonlocal_desc* d, const typename std::conditional<LSE, NlParamsLse, NlParams>::type& p) {
    if (d->dtype == DAT_BF16) {
        switch (d->D) {
            case 64: return nl_launch<DAT_BF16, 64, 64, LSE>(ctx, st, d, p);
            case 128: return nl_launch<DAT_BF16, 128, 128, LSE>(ctx, st, d, p);
            case 256: return nl_launch<DAT_BF16, 256, 256, LSE>(ctx, st, d, p);
            default: return nl_launch<DAT_BF16, 512, 256, LSE>(ctx, st, d, p);   // two value slices, scores recomputed per slice
        }
    }
    switch (d->D) {
        case 64: return nl_launch<DAT_F32, 64, 64, LSE>(ctx, st, d, p);
        case 128: return nl_launch<DAT_F32, 128, 128, LSE>(ctx, st, d, p);
        case 256: return nl_launch<DAT_F32, 256, 128, LSE>(ctx, st, d, p);
        default: return nl_launch<DAT_F32, 512, 64, LSE>(ctx, st, d, p);
    }
}

}  // namespace

extern "C" {

int dat_nonlocal_attention(dat_ctx* ctx, dat_stream s, const dat_nonlocal_desc* d, const void* q, const void* k, const void* v, void* y) {
    NlParams p;
    const int rc = nl_check(ctx, d, q, k, v, y, p);
    if (rc != DAT_OK) return rc;
    return nl_dispatch<false>(ctx, (hipStream_t)s, d, p);
}

// The same kernel, also storing lse[clip * Lq + i] = m_i + log2(l_i) (fp32, in the units of scale * log2(e) * score): what the backward
// (nonlocal_bwd.hip) recomputes P from.  y is bit-identical to dat_nonlocal_attention.
int dat_nonlocal_attention_lse(dat_ctx* ctx, dat_stream s, const dat_nonlocal_desc* d, const void* q, const void* k, const void* v, void* y,
                               float* lse) {
    NlParamsLse p;
    const int rc = nl_check(ctx, d, q, k, v, y, p);
    if (rc != DAT_OK) return rc;
    DAT_ENFORCE(ctx, lse && ((uintptr_t)lse & 3) == 0, "nonlocal_attention_lse: lse is null or misaligned (%p)", (void*)lse);
    p.lse = lse;
    return nl_dispatch<true>(ctx, (hipStream_t)s, d, p);
}

}  // extern "C"
