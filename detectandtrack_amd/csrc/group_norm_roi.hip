// GroupNorm on per-RoI blobs [R][rows][cstride] (rows = Tr * H * W positions of one RoI; the C4 res5 box head, the keypoint head):
// statistics and normalisation in ONE launch, the whole backward in one launch plus a small one for dbeta / dgamma.  DESIGN.md
// section 3.12.  A RoI is 49-1568 positions: one block of 1024 threads owns one RoI, all of its channels, and keeps the RoI's packed
// 16-byte vectors in registers between the passes (mean, then a true second pass for M2 = sum (z - mean)^2, then the normalise), so z is
// read from HBM once.  A RoI too large for the registers is split into channel slabs of whole groups, one block each (roi_slab: the
// groups are independent, so the blocks share nothing); a slab that still does not fit takes the same kernel with NV = 0, which
// re-reads its operands in every pass.  Groups of any cg = C / G, also ones that straddle 64-channel chunks: the block reduces per CHANNEL and a
// thread per group folds the group's channels in channel order.
//
//   thread layout (cstride: of the block's slab): cv = cstride / VEC threads cover one row with ONE 16-byte access each, RL = 1024 / cv row lanes; a thread keeps one
//   channel vector and the rows rl, rl + RL, ...  (threads past RL * cv idle: cstride 192 in fp32 leaves 16 of 1024)
//   reduction: thread (its rows in order) -> LDS [RL][cstride] -> a thread per channel sums the RL lanes in order -> a thread per group
//   sums its cg channels in order.  The order depends on (dtype, rows, C, cstride, groups) only: never on R, on which RoIs are
//   live, or on the launch -- a RoI gets the same bits alone and among others.  No float atomics.
//
// Dead RoIs (count != NULL and r % seg >= count[r / seg], seg = R / n_seg: the equal row segments per image of the RoI blobs): the
// block reads none of their inputs and writes zeros to every output row.  Padding channels [C, cstride) are written as zeros and
// never enter a sum (whatever they hold, NaN included, stays in partials nobody reads).
#include "norm_kernels.h"

namespace {

constexpr int GR_BLOCK = 1024;
constexpr int GR_U = 4;             // 16-byte loads in flight per thread and operand in the re-reading (NV = 0) passes: forward,
constexpr int GR_UB = 2;            // backward (three operands)
constexpr int GR_MAX_CS = 2048;     // LDS: (1024 * VEC + 2 * cstride) floats <= 48 KB
constexpr int GR_ML = 16, GR_SUM_BLOCK = 64 * GR_ML;

// the packed vector as a value the compiler knows nothing about: without it the unpacked floats of one pass are kept for the next
// (common subexpressions), VEC registers per vector instead of 4
__device__ __forceinline__ uint4 opaque(uint4 p) {
    asm volatile("" : "+v"(p.x), "+v"(p.y), "+v"(p.z), "+v"(p.w));
    return p;
}
// (register-to-register conversions: Vec<DT>::unpack / pack of norm_kernels.h)
template <int DT> __device__ __forceinline__ void unpack(const uint4& a, float* v) { Vec<DT>::unpack(a, v); }
template <int DT> __device__ __forceinline__ uint4 pack(const float* v) { return Vec<DT>::pack(v); }

// the thread's place in the layout of the file comment, and whether the block's RoI is live
template <int DT> struct RoiLane {
    static constexpr int VEC = Vec<DT>::N;
    int cv, rv, RL, cvi, rl, lc, c0, cbase, myrows;     // lc / c0: the thread's first channel within the slab / the blob; myrows: `rows`
    size_t roi, vbase;                                  // for a thread that has a row lane, 0 for an idle one; vbase: the slab's first vector
    bool live;
    // block b of the 1-D grid owns the channel slab [cbase, cbase + cw) (whole groups) of RoI b / (cs / cw)
    __device__ __forceinline__ RoiLane(int rows, int cs, int cw, const int* count, int seg) {
        const int S = cs / cw;
        roi = blockIdx.x / S;
        cbase = (int)(blockIdx.x % S) * cw;
        cv = cw / VEC;
        rv = cs / VEC;
        RL = GR_BLOCK / cv;
        cvi = threadIdx.x % cv;
        rl = threadIdx.x / cv;
        lc = cvi * VEC;
        c0 = cbase + lc;
        myrows = rl < RL ? rows : 0;
        vbase = roi * rows * rv + cbase / VEC;
        live = !count || (int)(roi % seg) < count[roi / seg];
    }
    __device__ __forceinline__ size_t at(int r) const { return vbase + (size_t)r * rv + cvi; }
    // a row the thread may always load: its own row r, or (past its rows, idle threads) row 0 of its channel vector.  The value loaded
    // for a row that is not the thread's is never used; with an output aliasing the input (y over z, g over dy) that location may be
    // written by the thread that owns row 0 at the same time -- harmless, because nothing depends on what this load returns.
    __device__ __forceinline__ size_t clamped(int r) const { return at(r < myrows ? r : 0); }
    __device__ __forceinline__ void zero_rows(void* p) const {
        uint4* o = (uint4*)p;
        for (int r = rl; r < myrows; r += RL) o[at(r)] = make_uint4(0, 0, 0, 0);
    }
};

// f(row, packed vector) on the thread's rows in order: from the registers (NV > 0: zr[k] is row rl + k * RL), else re-read from src
template <int DT, int NV, typename F>
__device__ __forceinline__ void each_row(const RoiLane<DT>& ln, const uint4* src, const uint4* zr, F f) {
    if constexpr (NV > 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int r = ln.rl + k * ln.RL;
            if (r < ln.myrows) f(r, opaque(zr[k]));
        }
    } else {
        for (int r = ln.rl; r < ln.myrows; r += ln.RL * GR_U) {
            uint4 t[GR_U];
#pragma unroll
            for (int u = 0; u < GR_U; ++u) t[u] = src[ln.clamped(r + u * ln.RL)];
#pragma unroll
            for (int u = 0; u < GR_U; ++u) {
                const int rr = r + u * ln.RL;
                if (rr < ln.myrows) f(rr, t[u]);
            }
        }
    }
}

// the threads' per-channel partials acc[VEC] -> tot[c], c < cs (here: the slab's width, channels local to the slab): the row lanes in
// order.  s_red: [RL][cs].  Ends with a barrier.
template <int DT>
__device__ __forceinline__ void channel_totals(const RoiLane<DT>& ln, const float* acc, int cs, float* s_red, float* tot) {
    constexpr int VEC = Vec<DT>::N;
    if (ln.rl < ln.RL) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) s_red[ln.rl * cs + ln.lc + e] = acc[e];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < cs; c += GR_BLOCK) {
        float t = s_red[c];
        for (int j = 1; j < ln.RL; ++j) t += s_red[j * cs + c];
        tot[c] = t;
    }
    __syncthreads();
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
template <int DT, int NV>
__global__ void __launch_bounds__(GR_BLOCK) gn_roi_fwd_kernel(const void* z, const void* res, void* y, int rows, int C, int cs, int G,
                                                              const float* __restrict__ scale, const float* __restrict__ bias, float eps,
                                                              int relu, float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                              const int* __restrict__ count, int seg, int cw) {
    constexpr int VEC = Vec<DT>::N;
    const RoiLane<DT> ln(rows, cs, cw, count, seg);
    extern __shared__ float smem[];
    float* s_red = smem;                        // [RL][cw] <= GR_BLOCK * VEC floats; then the groups' rstd
    float* s_tot = smem + GR_BLOCK * VEC;       // [cw] channel totals
    float* s_grp = s_tot + cw;                  // group means
    const size_t roi = ln.roi;
    const int cg = C / G;
    // the slab's groups [g_lo, g_lo + ng) (none when the slab is padding only)
    const int g_lo = (ln.cbase < C ? ln.cbase : C) / cg, ng = (ln.cbase + cw < C ? ln.cbase + cw : C) / cg - g_lo;
    if (!ln.live) {
        ln.zero_rows(y);
        for (int k = threadIdx.x; k < ng; k += GR_BLOCK) mean_out[roi * G + g_lo + k] = rstd_out[roi * G + g_lo + k] = 0.f;
        return;
    }
    const uint4* zv = (const uint4*)z;
    uint4 zr[NV > 0 ? NV : 1];
    if constexpr (NV > 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) zr[k] = zv[ln.clamped(ln.rl + k * ln.RL)];
    }
    const float Mg = (float)rows * (float)cg;
    int grp[VEC];       // the channel's group within the slab, -1: padding
#pragma unroll
    for (int e = 0; e < VEC; ++e) grp[e] = ln.c0 + e < C ? (ln.c0 + e) / cg - g_lo : -1;

    // pass 1: the mean
    float acc[VEC], mu[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    each_row<DT, NV>(ln, zv, zr, [&](int, const uint4& p) {
        float v[VEC];
        unpack<DT>(p, v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] += v[e];
    });
    channel_totals<DT>(ln, acc, cw, s_red, s_tot);
    for (int k = threadIdx.x; k < ng; k += GR_BLOCK) {
        const int cl = (g_lo + k) * cg - ln.cbase;
        float t = s_tot[cl];
        for (int c = cl + 1; c < cl + cg; ++c) t += s_tot[c];
        s_grp[k] = t / Mg;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < VEC; ++e) mu[e] = grp[e] >= 0 ? s_grp[grp[e]] : 0.f;

    // pass 2: M2 around that mean over the same values (never E[x^2] - mean^2)
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    each_row<DT, NV>(ln, zv, zr, [&](int, const uint4& p) {
        float v[VEC];
        unpack<DT>(p, v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float d = v[e] - mu[e];
            acc[e] = fmaf(d, d, acc[e]);
        }
    });
    channel_totals<DT>(ln, acc, cw, s_red, s_tot);
    for (int k = threadIdx.x; k < ng; k += GR_BLOCK) {
        const int cl = (g_lo + k) * cg - ln.cbase;
        float t = s_tot[cl];
        for (int c = cl + 1; c < cl + cg; ++c) t += s_tot[c];
        const float rstd = 1.f / sqrtf(t / Mg + eps);
        s_red[k] = rstd;
        mean_out[roi * G + g_lo + k] = s_grp[k];
        rstd_out[roi * G + g_lo + k] = rstd;
    }
    __syncthreads();

    // pass 3: y = act(z a + b' (+ res)), a = scale rstd, b' = bias - mean a: the form of the per-clip apply
    float ka[VEC], kb[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const int c = ln.c0 + e;
        ka[e] = grp[e] >= 0 ? scale[c] * s_red[grp[e]] : 0.f;
        kb[e] = grp[e] >= 0 ? bias[c] - mu[e] * ka[e] : 0.f;
    }
    const uint4* rv = (const uint4*)res;
    uint4* yv = (uint4*)y;
    each_row<DT, NV>(ln, zv, zr, [&](int r, const uint4& p) {
        float v[VEC], q[VEC];
        unpack<DT>(p, v);
        if (rv) unpack<DT>(rv[ln.at(r)], q);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            float o = fmaf(v[e], ka[e], kb[e]);
            if (rv) o += q[e];
            if (relu) o = o > 0.f ? o : 0.f;
            v[e] = grp[e] >= 0 ? o : 0.f;
        }
        yv[ln.at(r)] = pack<DT>(v);
    });
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------
// g = dy [y > 0];  sums[roi][0][c] = S1 = sum g,  sums[roi][1][c] = S2 = sum g xhat;  per group A = sum scale S1, B = sum scale S2;
// dz = a g + q + r (z - mean),  a = scale rstd,  q = -rstd A / Mg,  r = -rstd^2 B / Mg   ( = rstd (scale g - A / Mg - xhat B / Mg) ).
// NV > 0: the packed g and z stay in registers between the two passes; NV = 0: the second pass re-reads dy, y and z.
template <int DT, int NV>
__global__ void __launch_bounds__(GR_BLOCK) gn_roi_bwd_kernel(const void* dy, const void* y, const void* z, void* g, void* dz, int rows, int C,
                                                              int cs, int G, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              const float* __restrict__ scale, int relu, float* __restrict__ sums,
                                                              const int* __restrict__ count, int seg, int cw) {
    constexpr int VEC = Vec<DT>::N;
    const RoiLane<DT> ln(rows, cs, cw, count, seg);
    extern __shared__ float smem[];
    float* s_red = smem;                        // [RL][cw]; then the groups' q and r
    float* s_1 = smem + GR_BLOCK * VEC;         // [cw] S1
    float* s_2 = s_1 + cw;                      // [cw] S2
    const size_t roi = ln.roi;
    float* sums1 = sums + roi * 2 * cs + ln.cbase;      // the slab's channels of S1; S2 is cs further
    if (!ln.live) {
        if (g) ln.zero_rows(g);
        if (dz) ln.zero_rows(dz);
        for (int c = threadIdx.x; c < cw; c += GR_BLOCK) sums1[c] = sums1[cs + c] = 0.f;
        return;
    }
    const int cg = C / G;
    const int g_lo = (ln.cbase < C ? ln.cbase : C) / cg, ng = (ln.cbase + cw < C ? ln.cbase + cw : C) / cg - g_lo;
    const int nreal = C - ln.c0;     // the thread's channels e < nreal are real, the others padding
    float mu[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) mu[e] = e < nreal ? mean[roi * G + (ln.c0 + e) / cg] : 0.f;
    const uint4* dv = (const uint4*)dy;
    const uint4* yv = (const uint4*)y;
    const uint4* zv = (const uint4*)z;
    uint4* gv = (uint4*)g;
    float sb[VEC], ss[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) sb[e] = ss[e] = 0.f;
    // one row: the masked gradient (packed: dy or 0, exact in the tensor format) and its two partial sums
    auto reduce_row = [&](int r, const uint4& pd, const uint4& py, const uint4& pz, bool store) -> uint4 {
        float d[VEC], o[VEC], x[VEC];
        unpack<DT>(pd, d);
        unpack<DT>(pz, x);
        if (relu) unpack<DT>(py, o);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            if ((relu && !(o[e] > 0.f)) || e >= nreal) d[e] = 0.f;
            sb[e] += d[e];
            ss[e] = fmaf(d[e], x[e] - mu[e], ss[e]);      // (S2 = rstd sum g (z - mean): rstd is constant within the thread's channel)
        }
        const uint4 pg = pack<DT>(d);
        if (store && gv) gv[ln.at(r)] = pg;
        return pg;
    };
    uint4 gr[NV > 0 ? NV : 1], zr[NV > 0 ? NV : 1];
    if constexpr (NV > 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int r = ln.rl + k * ln.RL;
            const size_t at = ln.clamped(r);
            uint4 py = make_uint4(0, 0, 0, 0);
            gr[k] = dv[at];
            zr[k] = zv[at];
            if (relu) py = yv[at];
            if (r < ln.myrows) gr[k] = reduce_row(r, gr[k], py, zr[k], true);
        }
    } else {
        for (int r = ln.rl; r < ln.myrows; r += ln.RL * GR_UB) {
            uint4 td[GR_UB], ty[GR_UB], tz[GR_UB];
#pragma unroll
            for (int u = 0; u < GR_UB; ++u) {
                const size_t at = ln.clamped(r + u * ln.RL);
                td[u] = dv[at];
                tz[u] = zv[at];
                if (relu) ty[u] = yv[at];
            }
#pragma unroll
            for (int u = 0; u < GR_UB; ++u) {
                const int rr = r + u * ln.RL;
                if (rr < ln.myrows) reduce_row(rr, td[u], ty[u], tz[u], true);
            }
        }
    }
    float rs[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        rs[e] = e < nreal ? rstd[roi * G + (ln.c0 + e) / cg] : 0.f;
        ss[e] *= rs[e];
    }
    channel_totals<DT>(ln, sb, cw, s_red, s_1);
    channel_totals<DT>(ln, ss, cw, s_red, s_2);
    for (int c = threadIdx.x; c < cw; c += GR_BLOCK) {
        sums1[c] = ln.cbase + c < C ? s_1[c] : 0.f;
        sums1[cs + c] = ln.cbase + c < C ? s_2[c] : 0.f;
    }
    if (!dz) return;
    const float invMg = 1.f / ((float)rows * (float)cg);
    for (int k = threadIdx.x; k < ng; k += GR_BLOCK) {
        float A = 0.f, B = 0.f;
        for (int c = (g_lo + k) * cg; c < (g_lo + k + 1) * cg; ++c) {
            A = fmaf(scale[c], s_1[c - ln.cbase], A);
            B = fmaf(scale[c], s_2[c - ln.cbase], B);
        }
        const float r1 = rstd[roi * G + g_lo + k];
        s_red[k] = -(r1 * A) * invMg;
        s_red[cw + k] = -(r1 * r1 * B) * invMg;
    }
    __syncthreads();
    float ka[VEC], kq[VEC], kr[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const int k = (ln.c0 + e) / cg - g_lo;
        ka[e] = e < nreal ? scale[ln.c0 + e] * rs[e] : 0.f;
        kq[e] = e < nreal ? s_red[k] : 0.f;
        kr[e] = e < nreal ? s_red[cw + k] : 0.f;
    }
    uint4* dzv = (uint4*)dz;
    // (z - mean, not r z + (q - r mean): the difference is the small number, also for a RoI whose mean is far from zero)
    auto apply_row = [&](int r, const uint4& pg, const uint4& pz) {
        float gg[VEC], x[VEC];
        unpack<DT>(pg, gg);
        unpack<DT>(pz, x);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float o = fmaf(ka[e], gg[e], fmaf(kr[e], x[e] - mu[e], kq[e]));
            x[e] = e < nreal ? o : 0.f;
        }
        dzv[ln.at(r)] = pack<DT>(x);
    };
    if constexpr (NV > 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int r = ln.rl + k * ln.RL;
            if (r < ln.myrows) apply_row(r, opaque(gr[k]), opaque(zr[k]));
        }
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) sb[e] = ss[e] = 0.f;      // (reduce_row keeps summing: unused from here on)
        for (int r = ln.rl; r < ln.myrows; r += ln.RL * GR_UB) {
            uint4 td[GR_UB], ty[GR_UB], tz[GR_UB];
#pragma unroll
            for (int u = 0; u < GR_UB; ++u) {
                const size_t at = ln.clamped(r + u * ln.RL);
                td[u] = dv[at];
                tz[u] = zv[at];
                if (relu) ty[u] = yv[at];
            }
#pragma unroll
            for (int u = 0; u < GR_UB; ++u) {
                const int rr = r + u * ln.RL;
                if (rr < ln.myrows) apply_row(rr, reduce_row(rr, td[u], ty[u], tz[u], false), tz[u]);
            }
        }
    }
}

// dbeta[c] += sum_r sums[r][0][c], dgamma[c] += sum_r sums[r][1][c] (dead RoIs hold zeros): grid (chunks), GR_ML lanes per channel;
// lane l sums the RoIs l, l + GR_ML, ... in order into its row of the workspace ([GR_ML][2][cs]), lane 0 then sums the lanes in
// order.  The order depends on R only.
__global__ void __launch_bounds__(GR_SUM_BLOCK) gn_roi_param_grads_kernel(const float* __restrict__ sums, int R, int cs, int C,
                                                                          float* part, float* __restrict__ dbeta,
                                                                          float* __restrict__ dgamma) {
    const int cl = threadIdx.x & 63, lane = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    float b = 0.f, s = 0.f;
#pragma unroll 4
    for (int r = lane; r < R; r += GR_ML) {
        b += sums[((size_t)r * 2) * cs + c];
        s += sums[((size_t)r * 2 + 1) * cs + c];
    }
    part[(lane * 2) * cs + c] = b;
    part[(lane * 2 + 1) * cs + c] = s;
    __syncthreads();
    if (lane != 0 || c >= C) return;
    for (int j = 1; j < GR_ML; ++j) {
        b += part[(j * 2) * cs + c];
        s += part[(j * 2 + 1) * cs + c];
    }
    if (dbeta) dbeta[c] += b;
    if (dgamma) dgamma[c] += s;
}

// row slots a thread needs to keep a slab of cw channels of the RoI in registers
int roi_slots(int dtype, int rows, int cw) {
    const int vec = dtype == DAT_BF16 ? Vec<DAT_BF16>::N : Vec<DAT_F32>::N;
    const int rl = GR_BLOCK / (cw / vec);
    return (rows + rl - 1) / rl;
}

size_t roi_lds_bytes(int dtype, int cw) {
    const int vec = dtype == DAT_BF16 ? Vec<DAT_BF16>::N : Vec<DAT_F32>::N;
    return ((size_t)GR_BLOCK * vec + 2 * (size_t)cw) * sizeof(float);
}

// Channels per block.  A RoI that fits the largest resident instantiation (`limit` row slots) stays whole: one block, cw = cs.  A larger
// one is halved into slabs of whole groups -- the groups are independent, so the blocks of a RoI share nothing -- until a slab fits or
// a row of the slab would be shorter than 128 bytes; the narrower slab also has more row lanes, i.e. fewer rows per thread.  A function
// of (dtype, rows, C, cs, groups) only, like everything else that fixes the summation order.
int roi_slab(int dtype, int rows, int C, int cs, int groups, int limit) {
    const int esize = dtype == DAT_BF16 ? 2 : 4, vec = 16 / esize, cg = C / groups;
    int cw = cs;
    while (roi_slots(dtype, rows, cw) > limit && cw % 2 == 0 && (cw / 2) % cg == 0 && (cw / 2) % vec == 0 && (cw / 2) * esize >= 128) cw /= 2;
    return cw;
}

int gn_roi_check(dat_ctx* ctx, const char* what, int dtype, int R, long long rows, int C, int cs, int groups, const int* count, int n_seg) {
    DAT_ENFORCE(ctx, dtype == DAT_F32 || dtype == DAT_BF16, "%s: dtype %d", what, dtype);
    DAT_ENFORCE(ctx, R >= 1 && R <= (1 << 24), "%s: %d RoIs", what, R);
    DAT_ENFORCE(ctx, cs >= 64 && cs % 64 == 0 && cs <= GR_MAX_CS && C >= 1 && C <= cs,
                "%s: %d channels at stride %d (a multiple of 64, at most %d)", what, C, cs, GR_MAX_CS);
    DAT_ENFORCE(ctx, rows >= 1 && rows * (long long)cs < (1ll << 31) && rows * (long long)cs < (1ll << 40) / R, "%s: %d RoIs of %lld rows",
                what, R, rows);
    DAT_ENFORCE(ctx, groups >= 1 && C % groups == 0, "%s: %d channels in %d groups", what, C, groups);
    DAT_ENFORCE(ctx, rows * (C / groups) >= 2, "%s: group statistics need at least 2 values per group (got %lld)", what,
                rows * (C / groups));
    DAT_ENFORCE(ctx, n_seg >= 1 && R % n_seg == 0, "%s: %d RoIs do not split into %d equal row segments", what, R, n_seg);
    DAT_ENFORCE(ctx, ((uintptr_t)count & 3) == 0, "%s: count must be 4-byte aligned", what);
    return DAT_OK;
}

}  // namespace

// NV: the smallest instantiated number of row slots that holds the RoI, 0 (re-read) beyond the largest that compiles without spills
#define GR_LAUNCH(kern, DT, NV, ...) hipLaunchKernelGGL((kern<DT, NV>), dim3(blocks), dim3(GR_BLOCK), lds, (hipStream_t)s, __VA_ARGS__)

size_t dat_gn_roi_workspace_bytes(int R, int cstride) {
    if (R < 1 || R > (1 << 24) || cstride < 64 || cstride % 64 != 0 || cstride > GR_MAX_CS) return 0;
    return (size_t)GR_ML * 2 * cstride * sizeof(float);
}

int dat_gn_roi_fwd(dat_ctx* ctx, dat_stream s, int dtype, const void* z, const void* residual, void* y, int R, long long rows, int C,
                   int cstride, int groups, const float* scale, const float* bias, float eps, int relu, float* mean, float* rstd,
                   const int* count, int n_seg) {
    const int rc = gn_roi_check(ctx, "gn_roi_fwd", dtype, R, rows, C, cstride, groups, count, n_seg);
    if (rc != DAT_OK) return rc;
    DAT_ENFORCE(ctx, z && y && scale && bias && mean && rstd, "gn_roi_fwd: null argument");
    DAT_ENFORCE(ctx, aligned16(z) && aligned16(y) && aligned16(residual), "gn_roi_fwd: tensors must be 16-byte aligned");
    const int cw = roi_slab(dtype, (int)rows, C, cstride, groups, dtype == DAT_BF16 ? 13 : 20);
    const int need = roi_slots(dtype, (int)rows, cw), seg = R / n_seg, blocks = R * (cstride / cw);
    const size_t lds = roi_lds_bytes(dtype, cw);
#define GR_FWD(DT, NV) GR_LAUNCH(gn_roi_fwd_kernel, DT, NV, z, residual, y, (int)rows, C, cstride, groups, scale, bias, eps, relu, mean, rstd, count, seg, cw)
    if (dtype == DAT_BF16) {
        if (need <= 4) GR_FWD(DAT_BF16, 4);
        else if (need <= 10) GR_FWD(DAT_BF16, 10);
        else if (need <= 13) GR_FWD(DAT_BF16, 13);
        else GR_FWD(DAT_BF16, 0);
    } else {
        if (need <= 4) GR_FWD(DAT_F32, 4);
        else if (need <= 10) GR_FWD(DAT_F32, 10);
        else if (need <= 20) GR_FWD(DAT_F32, 20);
        else GR_FWD(DAT_F32, 0);
    }
#undef GR_FWD
    DAT_CHECK_LAUNCH(ctx, "gn_roi_fwd");
    return DAT_OK;
}

int dat_gn_roi_bwd(dat_ctx* ctx, dat_stream s, int dtype, const void* dy, const void* y, const void* z, const float* mean, const float* rstd,
                   const float* scale, int R, long long rows, int C, int cstride, int groups, int relu, const int* count, int n_seg,
                   void* g, void* dz, float* sums, float* dbeta, float* dgamma, void* ws, size_t ws_bytes) {
    const int rc = gn_roi_check(ctx, "gn_roi_bwd", dtype, R, rows, C, cstride, groups, count, n_seg);
    if (rc != DAT_OK) return rc;
    DAT_ENFORCE(ctx, dy && z && mean && rstd && scale && sums && ws && (y || !relu), "gn_roi_bwd: null argument");
    DAT_ENFORCE(ctx, aligned16(dy) && aligned16(y) && aligned16(z) && aligned16(g) && aligned16(dz) && aligned16(ws),
                "gn_roi_bwd: tensors must be 16-byte aligned");
    const size_t need_ws = dat_gn_roi_workspace_bytes(R, cstride);
    DAT_ENFORCE(ctx, ws_bytes >= need_ws, "gn_roi_bwd: workspace of %zu bytes, %zu needed", ws_bytes, need_ws);
    const int cw = roi_slab(dtype, (int)rows, C, cstride, groups, dtype == DAT_BF16 ? 7 : 10);
    const int need = roi_slots(dtype, (int)rows, cw), seg = R / n_seg, blocks = R * (cstride / cw);
    const size_t lds = roi_lds_bytes(dtype, cw);
#define GR_BWD(DT, NV) GR_LAUNCH(gn_roi_bwd_kernel, DT, NV, dy, y, z, g, dz, (int)rows, C, cstride, groups, mean, rstd, scale, relu, sums, count, seg, cw)
    if (dtype == DAT_BF16) {
        if (need <= 4) GR_BWD(DAT_BF16, 4);
        else if (need <= 7) GR_BWD(DAT_BF16, 7);
        else GR_BWD(DAT_BF16, 0);
    } else {
        if (need <= 4) GR_BWD(DAT_F32, 4);
        else if (need <= 10) GR_BWD(DAT_F32, 10);
        else GR_BWD(DAT_F32, 0);
    }
#undef GR_BWD
    if (dbeta || dgamma)
        hipLaunchKernelGGL(gn_roi_param_grads_kernel, dim3(cstride / 64), dim3(GR_SUM_BLOCK), 0, (hipStream_t)s, (const float*)sums, R, cstride,
                           C, (float*)ws, dbeta, dgamma);
    DAT_CHECK_LAUNCH(ctx, "gn_roi_bwd");
    return DAT_OK;
}
