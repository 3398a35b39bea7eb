// Grouped 3D convolution (ResNeXt `branch2b`: kT x 3 x 3, C -> C in G groups of cg = C / G channels) for gfx950: the forward kernel with
// the shared fused epilogue (conv_epilogue.h: affine scale / bias, residual Sum or mask, ReLU) -- which, with the weights of
// dat_conv3d_grouped_pack_weights_dgrad, is also the data gradient -- and the weight-gradient kernel further down.  DESIGN.md section 3.8.
//
// The slab rule: an activation row in LDS is one 128-byte line = 64 bf16 channels, and for cg | 64 no group straddles a 64-channel slab.
// The layer is therefore C / 64 independent 64 -> 64 convs: the block that owns output channels [64 s, 64 s + 64) stages ONLY the
// input lines of slab s (bf16: one line per pixel, fp32: two 32-channel lines, bf16x3: the hi and the lo line of the split tensor) and
// multiplies them by a packed 64 x 64 x taps weight image that is block-diagonal inside the slab (64 / cg blocks of cg x cg, zeros
// elsewhere).  HBM traffic is the algorithmic minimum -- every input line is read by exactly one channel block per tile (plus halo),
// the weights are C * 64 * taps elements instead of C * C * taps -- and the MFMA utilisation is cg / 64 by construction.
//
// The main loop is the dense implicit-GEMM kernel's table-driven one (conv3d_igemm.hip): LDS-DMA patch staging of tile + halo per (kt,
// chunk, stride-parity plane), the ((row >> 1) & 7) XOR swizzle of the 16-byte slots, weights in MFMA A-fragment order straight from
// global memory into registers.  The block map and the LDS-transposed epilogue are the helpers of conv_epilogue.h, the tile, tap table
// and frame windows those of conv_internal.h.  One variant: 64 channels x 256 positions per block, every wave 64 channels x 64
// positions (stride 1: one plane of 9 taps; stride 2: four parity planes).
#include "conv_internal.h"

using namespace dat_conv;

namespace {

constexpr int G_BN = 64;       // output channels per block = one slab
constexpr int G_BP = 256;      // output positions per block
constexpr int G_BP_LOG2 = 8;

#define DAT_GRP_UNSUPPORTED(ctx, cond, ...)                          \
    do {                                                             \
        if (!(cond)) DAT_FAIL(ctx, DAT_ERR_UNSUPPORTED, __VA_ARGS__); \
    } while (0)

// ConvParams as the dense kernel reads them, with two fields re-read: n_cchunks = K chunks of ONE slab (bf16 1, fp32 2, bf16x3 3) and
// nblk_n = slabs (C / 64).  ksplit is 1, lin_* / order / res2 / part are unused.
// MASK: the residual operand masks instead of adding (res_mode 3, the data-gradient layer of training: y = residual > 0 ? v : 0) -- an
// instantiation of its own, so the inference instantiations keep their registers and their code.
template <int DT, int ODT, bool MASK = false>
__global__ __launch_bounds__(NTHREADS, 2) void conv3d_grouped_kernel(const ConvParams p) {
    constexpr int ES = ElemOf<DT>::size;
    constexpr int OES = ElemOf<ODT>::size;
    constexpr int WN = G_BN;              // channels per wave (all four waves share the slab)
    constexpr int WP = G_BP / 4;          // positions per wave
    constexpr int MT = WN / 32;
    constexpr int PT = WP / 32;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* patch = smem;                                      // PH*PW x 128 B

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // ---- XCD-aware block -> (slab, tile) map (bijective for any grid size): the slabs of one tile and neighbouring tiles share an XCD
    const unsigned bid = xcd_block_map(blockIdx.x, p.nblocks);
    const int slab = bid % p.nblk_n;
    unsigned tile = bid / p.nblk_n;
    const int fc = tile % p.otn;             // frame index fastest: the temporal re-reads of neighbouring output frames meet in the XCD's L2
    tile /= p.otn;
    const int tw_i = tile % p.tiles_w;
    tile /= p.tiles_w;
    const int th_i = tile % p.tiles_h;
    const int clip = tile / p.tiles_h;
    const int f = clip * p.otn + fc;         // output frame
    const int t = p.ot0 + fc;
    const int f_in = clip * p.T + t;         // input frame aligned with this output frame
    const int n0 = slab * G_BN;
    const int TW = 1 << p.tw_log2;
    const int oh0 = th_i << p.th_log2;
    const int ow0 = tw_i * p.tile_w;
    const int ih0 = oh0 * p.sh - p.ph;       // input coordinate of patch cell (0,0)
    const int iw0 = ow0 * p.sw - p.pw;

    int rowbase[PT];
#pragma unroll
    for (int j = 0; j < PT; ++j) {
        const int pos = wave * WP + j * 32 + (lane & 31);
        const int ohl = pos >> p.tw_log2, owl = pos & (TW - 1);
        rowbase[j] = ohl * p.PW + owl;
    }
    const int khalf = lane >> 5;

    f32x16_t acc[MT][PT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < PT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // valid temporal taps for this output frame (a tap outside the clip reads zeros: skipped)
    int kt_lo = 0, kt_hi = p.KT - 1;
    while (kt_lo < p.KT && (t + kt_lo - p.pt) < p.in_lo) ++kt_lo;
    while (kt_hi >= 0 && (t + kt_hi - p.pt) >= p.in_hi) --kt_hi;
    const int n_kt = kt_hi - kt_lo + 1;
    const int ntap = p.KH * p.KW;
    const int ntab = p.tab_n;
    const int total = n_kt * p.n_cchunks * ntab;           // tap steps
    const int npatch_items = p.PH * p.PW * 8;

    typedef const __attribute__((address_space(1))) void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;

    // this wave's A fragments: 4 KiB per (tap, slab chunk, 32-row block), this lane's 16 B inside it
    const size_t wd_cc_stride = (size_t)(p.Cout_pad >> 5) * 4096;
    const char* const wd_lane = p.w + (size_t)(n0 >> 5) * 4096 + lane * 16;
#define WD_PTR(KT_, CC_, TI_) (wd_lane + ((size_t)((KT_) * ntap + p.tab_tap[(TI_)]) * p.n_cchunks + (CC_)) * wd_cc_stride)
    if (total > 0) {
        // temporal taps in order of the INPUT frame index mod KT (see the dense kernel): queue neighbours stage the same frame together
        const int kt_hi_x = kt_lo + n_kt;
        int kshift = 0;
        if (n_kt == p.KT && (DAT_KT_ROTATE)) kshift = (p.KT - (t + kt_lo - p.pt) % p.KT) % p.KT;
        int kt = kt_lo + kshift, cc = 0, ti = 0;
        if (kt >= kt_hi_x) kt -= n_kt;
        uint4 wa[MT][4];
        {
            const char* w0 = WD_PTR(kt, cc, 0);
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) wa[i][ks] = *(const uint4*)(w0 + i * 4096 + ks * 1024);
        }
        const int nchunks = (npatch_items + 63) >> 6;    // 1-KiB LDS-DMA pieces (8 patch rows each)
        for (int step = 0; step < total; ++step) {
            const bool reload = (p.tab_new >> ti) & 1u;
            // (bf16x3, one stride plane: chunk 1 -- x_hi against W_lo -- re-uses the patch of chunk 0)
            const bool x3_same = p.x3 && p.tab_new == 1u && step > 0 && cc == 1;
            if (reload && !x3_same) {
                __syncthreads();  // all waves finished reading the previous patch
                // ---- stage the input patch (tile + halo) of (kt, slab chunk, plane): global -> LDS by LDS-DMA.  Lane (row, phys slot)
                // fetches the pixel's logical 16-B slot phys ^ ((row >> 1) & 7); halo pixels outside the frame fetch zeros.  Only the
                // 128-byte lines of THIS slab are read: line slab * chunks + cc of the pixel (bf16x3: 2 * slab = hi, 2 * slab + 1 = lo).
                const int fin = f_in + kt - p.pt;
                const int line = p.x3 ? slab * 2 + (cc == 2) : slab * p.n_cchunks + cc;
                const char* xbase = p.x + ((size_t)fin * p.H * p.W) * p.Cin * ES + (size_t)line * PPITCH;
                const int py0 = ih0 + p.tab_dy[ti], px0 = iw0 + p.tab_dx[ti];
#pragma unroll 2
                for (int c = wave; c < nchunks; c += 4) {
                    const int it = c * 64 + lane;
                    if (it < npatch_items) {
                        const int row = it >> 3;
                        const int slot = (it ^ (row >> 1)) & 7;
                        const int prow = (int)__umulhi((unsigned)row, p.pw_magic), pcol = row - prow * p.PW;   // (PW >= 2: pw_magic != 0)
                        const int ih = py0 + prow * p.psh, iw = px0 + pcol * p.psw;
                        const char* src = p.zeros;
                        if (ih >= 0 && ih < p.H && iw >= 0 && iw < p.W)
                            src = xbase + ((unsigned)(ih * p.W + iw) * (unsigned)(p.Cin * ES) + (unsigned)(slot * 16));
                        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(patch + c * 1024), 16, 0, 0);
                    }
                }
            }
            if (reload) {   // only a patch reload needs the block to meet (a ds_read is ordered behind an LDS-DMA by vmcnt + a barrier)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
            }
            int nti = ti + 1, ncc = cc, nkt = kt;
            if (nti == ntab) {
                nti = 0;
                if (++ncc == p.n_cchunks) { ncc = 0; if (++nkt == kt_hi_x) nkt = kt_lo; }
            }
            const char* const wnext = (step + 1 < total) ? WD_PTR(nkt, ncc, nti) : WD_PTR(kt, cc, ti);

            __builtin_amdgcn_s_setprio(1);
            {
                const int tapoff = p.tab_rowoff[ti];
                // patch fragment of (row, k-slice ks, k-half): 16-B slot (2*ks + khalf) ^ ((row >> 1) & 7) of the row's line
                const char* bp[PT];
                int bx[PT];
#pragma unroll
                for (int j = 0; j < PT; ++j) {
                    const int row = rowbase[j] + tapoff;
                    const int g = (row >> 1) & 7;
                    bp[j] = patch + (row * PPITCH + ((khalf ^ (g & 1)) << 4));
                    bx[j] = g >> 1;
                }
                uint4 b[2][PT];
#pragma unroll
                for (int j = 0; j < PT; ++j) b[0][j] = *(const uint4*)(bp[j] + (bx[j] << 5));
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const int cur = ks & 1, nxt = cur ^ 1;
                    if (ks < 3) {
#pragma unroll
                        for (int j = 0; j < PT; ++j) b[nxt][j] = *(const uint4*)(bp[j] + (((ks + 1) ^ bx[j]) << 5));
                    }
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int j = 0; j < PT; ++j) Mma<DT>::step(wa[i][ks], b[cur][j], acc[i][j]);
                    // this k-slice's fragments of the NEXT tap: a whole tap to land (unconditional and pinned, see the dense kernel)
#pragma unroll
                    for (int i = 0; i < MT; ++i) wa[i][ks] = *(const uint4*)(wnext + i * 4096 + ks * 1024);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            __builtin_amdgcn_s_setprio(0);
            ti = nti; cc = ncc; kt = nkt;
        }
    }
#undef WD_PTR

    // ---- epilogue (conv_epilogue.h): the dense kernel's without split-K, channel tail (Cout is a multiple of 64) and masking modes;
    // the residual row is loaded where it is added ----
    constexpr int CPL = 16 / OES;                 // channels per lane in the store phase (8 bf16 / 4 fp32)
    constexpr int LPP = WN / CPL;                // lanes per position (8 / 16)
    constexpr int PPI = 64 / LPP;                // positions per store instruction (8 / 4)
    __syncthreads();                             // every wave is done with the patch
    char* est = smem + wave * (32 * EPI_PITCH);
    const int sl_c = (lane % LPP) * CPL, sl_p = lane / LPP;
    const int c_st = n0 + sl_c;
    float sc[CPL], bi[CPL];
#pragma unroll
    for (int e = 0; e < CPL; ++e) {
        sc[e] = p.scale ? p.scale[c_st + e] : 1.f;
        bi[e] = p.bias ? p.bias[c_st + e] : 0.f;
    }
    // block-uniform 64-bit base + 32-bit per-lane offset inside the frame (the launcher checks one frame of output is < 2 GB)
    const size_t tile_pos = ((size_t)f * p.Ho + oh0) * p.Wo + ow0;
    char* const ybase = p.y + tile_pos * p.out_cs * OES;
    const char* const rbase = p.res + tile_pos * p.out_cs * OES;
#pragma unroll
    for (int j = 0; j < PT; ++j) {
#pragma unroll
        for (int i = 0; i < MT; ++i) epi_stage(est, lane & 31, khalf, i, acc[i][j]);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q = 0; q < 32 / PPI; ++q) {
            const int pl = q * PPI + sl_p;
            float v[CPL];
            epi_load(est, pl, sl_c, v);
            const int pos = wave * WP + j * 32 + pl;
            const int ohl = pos >> p.tw_log2, owl = pos & (TW - 1);
            if (oh0 + ohl >= p.Ho || ow0 + owl >= p.Wo) continue;
            const unsigned lpos = (unsigned)(ohl * p.Wo + owl);
            const unsigned off = (lpos * (unsigned)p.out_cs + (unsigned)c_st) * (unsigned)OES;
            epi_affine(v, sc, bi);
            if (MASK || p.res_mode) epi_residual<ODT>(v, *(const uint4*)(rbase + off), MASK ? 3 : 1);
            epi_relu(v, p.relu);
            epi_store<ODT>(ybase + off, v);
            // bf16x3: 64-channel chunk q of the pixel: line 2q = hi, line 2q + 1 = lo; this lane's 4 channels = 8 bytes in each line
            if (ODT == DAT_F32 && DT == DAT_BF16 && p.y_split)
                split_hi_lo_store(p.y_split + ((tile_pos + lpos) * (size_t)(2 * p.out_cs) + (size_t)((c_st >> 6) * 128 + (c_st & 63))) * 2, v);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// Packed grouped weights: the dense kernel's A-fragment order of a "64 -> C" conv -- [tap][slab chunk][32-row block][k-slice][lane][16 B],
// lane = k-half * 32 + row, 16-B slot (2 * k-slice + k-half) of the row's 128-B chunk -- whose row co holds, at the slab-local input
// channels of its own group, w[co][0 .. cg); zeros elsewhere (the block-diagonal 64 x 64 image) and in the rows past C.
// x3: three bf16 chunks [W_hi | W_lo | W_hi] per slab, met in the kernel by the input lines [hi | hi | lo].
// dgrad: the weights of the DATA-GRADIENT conv straight from the forward master: row ci (an input channel of the forward conv) holds,
// at the slab-local channels co of its own group, w[co][ci % cg][ntap - 1 - tap] * scale[co] -- the forward filter flipped over the
// taps, transposed inside each group, the fused AffineChannelNd scale folded in (grouped counterpart of conv_pack.hip's dgrad mode).
template <int DT>
__global__ void grouped_pack_kernel(const float* __restrict__ w, void* __restrict__ out, int C, int cg, int ntap, int Cout_pad, int nck, int x3,
                                    int dgrad, const float* __restrict__ scale) {
    constexpr int CK = Mma<DT>::CK, EPS = 16 / ElemOf<DT>::size;
    const size_t total = (size_t)ntap * nck * Cout_pad * CK;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int cl = i % CK;
        const int co = (i / CK) % Cout_pad;
        const int cc = (i / ((size_t)CK * Cout_pad)) % nck;
        const int tap = i / ((size_t)CK * Cout_pad * nck);
        const int j = x3 ? cl : cc * CK + cl;             // input channel inside the slab
        float v = 0.f;
        if (co < C) {
            const int cil = j - ((co & 63) / cg) * cg;    // ... inside the row's group
            if (cil >= 0 && cil < cg) {
                if (dgrad) {
                    const int cof = (co / cg) * cg + cil;     // forward output channel: this row's group, slab-local column
                    v = w[((size_t)cof * cg + co % cg) * ntap + (ntap - 1 - tap)] * (scale ? scale[cof] : 1.f);
                } else {
                    v = w[((size_t)co * cg + cil) * ntap + tap];
                }
            }
        }
        if (x3) {
            const float hi = bf2f(f2bf(v));
            v = cc == 1 ? v - hi : hi;
        }
        const int slot = cl / EPS, e = cl % EPS;
        const int lane = (slot & 1) * 32 + (co & 31);
        const size_t dst = (((((size_t)tap * nck + cc) * (Cout_pad >> 5) + (co >> 5)) * 4 + (slot >> 1)) * 64 + lane) * EPS + e;
        ElemOf<DT>::st(out, dst, v);
    }
}

// ---- weight gradient: dW[co][cil][kt][kh][kw] = sum_p g[p][co] * x[p (+) tap][(co / cg) * cg + cil] ------------------------------------------
// Per 64-channel slab a 64 x 64 x taps GEMM over the positions of which only the 64 / cg diagonal cg x cg blocks are kept.  The slab rule
// of the forward kernel holds here too: a block (slab, kt, range of position chunks) stages ONLY the slab's lines of g and x -- one
// 128-byte line per pixel in 16-bit, the 256 contiguous bytes of two 32-channel lines in fp32 -- by LDS-DMA, positions as LDS rows:
//   * a chunk = one 8 x 8 patch of output positions of one frame: 64 g rows, and the (7 s + 3)^2 input positions around it (s = 1: 10 x 10,
//     s = 2: 17 x 17) ONCE for all nine spatial taps; tap (kh, kw) of output (oy, ox) is patch row (s oy + kh) * PW + s ox + kw;
//   * 16-bit: the fragments are transposing reads (ds_read_b64_tr_b16; every lane supplies its own row address, so the stride-2 rows two
//     apart need no second layout) of rows swizzled as in wgrad_dma9_kernel -- 16-byte piece q of row r sits in slot q ^ 4 * bit1(r),
//     applied on the source side of the DMA: four consecutive rows x 64 B cover all 64 banks (stride 2: rows two apart, two-way);
//   * fp32 (the parity mode): plain ds_read_b32 operands of v_mfma_f32_32x32x2_f32, two positions per instruction;
//   * wave w of the four: cg = 64 -> quadrant (w & 1, w >> 1) of the slab over all 64 positions; cg <= 32 -> only the two DIAGONAL 32 x 32
//     quadrants hold kept blocks: quadrant w & 1 over positions [32 (w >> 1), + 32) of the chunk.  Nine accumulators (144 registers);
//   * the partial sums are ADDED to Gt[tap][C][cg] with float atomics, kept elements only -- products outside the diagonal blocks have no
//     address in that layout.
// Temporal taps outside the clip are skipped per chunk.  Every loop is bounded by launch arguments.
struct GWgradParams {
    const char* g;
    const char* x;
    float* G;                 // [KT * 9][C][cg] fp32
    const char* zeros;
    int C, cg_log2, g_cs;
    int T, H, W, Ho, Wo;
    int KT, pt;
    int nslab, ksplit, frames;
    int tiles_h, tiles_w;     // 8 x 8 output patches per frame
};

typedef short gw_v4s __attribute__((ext_vector_type(4)));

template <int DT, int S>
__global__ __launch_bounds__(NTHREADS, 2) void wgrad_grouped_kernel(const GWgradParams p) {
    constexpr int ES = ElemOf<DT>::size;
    constexpr int ROWB = 64 * ES;                 // one slab of one pixel: 128 B (16-bit) | 256 B (fp32)
    constexpr int SPR = ROWB / 16;                // 16-byte DMA slots per row
    constexpr int PW = 7 * S + 3;                 // input patch edge
    constexpr int PR = PW * PW;
    constexpr int RPP = 1024 / ROWB;              // rows per 1-KiB DMA piece
    constexpr int NROWS = (64 + PR + RPP - 1) / RPP * RPP;
    constexpr int NPIECES = NROWS / RPP;
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    typedef const __attribute__((address_space(1))) void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned bid = blockIdx.x;
    const int kt = bid % p.KT; bid /= p.KT;
    const int slab = bid % p.nslab;
    const int split = bid / p.nslab;
    const bool full = p.cg_log2 == 6;
    const int qm = wave & 1, qn = full ? wave >> 1 : qm;
    const int ks0 = full ? 0 : 2 * (wave >> 1), ks1 = full ? 4 : ks0 + 2;     // 16-position slices of the chunk
    const unsigned per_frame = (unsigned)(p.tiles_h * p.tiles_w);
    const unsigned nchunks = (unsigned)p.frames * per_frame;
    const unsigned c_lo = (unsigned)((unsigned long long)nchunks * split / p.ksplit);
    const unsigned c_hi = (unsigned)((unsigned long long)nchunks * (split + 1) / p.ksplit);
    const int khalf = lane >> 5, l31 = lane & 31;

    f32x16_t acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    // 16-bit fragment addressing: lane 4 q + c of a 16-lane group supplies row q, columns 4 c .. 4 c + 3 of a 4-row x 16-channel block and
    // receives channel (lane & 15) of the four rows.  Groups 0 / 1 = channels 0-15 / 16-31 of the quadrant, groups 2 / 3 the same of the
    // next eight positions (the k-half of the MFMA); the second read, four positions on, completes the lane's eight k.
    const int li = lane & 15, frow = li >> 2;
    const int fcol = ((((lane >> 4) & 1) * 16 + (li & 3) * 4) * 2);            // byte column inside the quadrant's 64 B
    char* const xs = smem + 64 * ROWB;
    typedef __attribute__((address_space(3))) gw_v4s* lp_t;
    auto tr4 = [&](const char* a) __attribute__((always_inline)) { return __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp_t)a)); };
    auto frag16 = [&](const char* base, int row, int rstep, int colb) __attribute__((always_inline)) {
        const int r1 = row + 4 * rstep;
        const uint2 lo = tr4(base + row * ROWB + (colb ^ ((row & 2) << 5)));
        const uint2 hi = tr4(base + r1 * ROWB + (colb ^ ((r1 & 2) << 5)));
        return make_uint4(lo.x, lo.y, hi.x, hi.y);
    };

    bool any = false;
    for (unsigned ch = c_lo; ch < c_hi; ++ch) {
        const unsigned fr = ch / per_frame, tl = ch - fr * per_frame;
        const int f = (int)fr;
        const int clip = f / p.T, t = f - clip * p.T, ti = t + kt - p.pt;
        if (ti < 0 || ti >= p.T) continue;                 // (block-uniform) the tap reads a frame outside the clip: zeros
        const int ty = (int)(tl / (unsigned)p.tiles_w), tx = (int)tl - ty * p.tiles_w;
        const int oy0 = ty * 8, ox0 = tx * 8;
        const int iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;
        const char* const gfr = p.g + (size_t)f * p.Ho * p.Wo * p.g_cs * ES + (size_t)slab * ROWB;
        const char* const xfr = p.x + (size_t)(clip * p.T + ti) * p.H * p.W * p.C * ES + (size_t)slab * ROWB;
        any = true;
        __syncthreads();                                   // every wave is done with the previous chunk's rows
        for (int c = wave; c < NPIECES; c += 4) {
            const int it = c * 64 + lane;
            const int row = it / SPR;
            int slot = it % SPR;
            if (ES == 2) slot ^= ((row >> 1) & 1) << 2;    // the bank swizzle of the transposing reads, on the source side
            const char* src = p.zeros;
            if (row < 64) {
                const int y = oy0 + (row >> 3), xq = ox0 + (row & 7);
                if (y < p.Ho && xq < p.Wo) src = gfr + ((size_t)y * p.Wo + xq) * p.g_cs * ES + slot * 16;
            } else if (row < 64 + PR) {
                const int xr = row - 64, py = xr / PW, px = xr - py * PW;
                const int y = iy0 + py, xq = ix0 + px;
                if (y >= 0 && y < p.H && xq >= 0 && xq < p.W) src = xfr + ((size_t)y * p.W + xq) * p.C * ES + slot * 16;
            }
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(smem + c * 1024), 16, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int ks = ks0; ks < ks1; ++ks) {
            if (ES == 2) {
                const int oy = 2 * ks + khalf;             // the eight k of this lane: output row oy, columns 0 .. 7
                const uint4 a = frag16(smem, oy * 8 + frow, 1, qm * 64 + fcol);
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        const uint4 b = frag16(xs, (S * oy + kh) * PW + S * frow + kw, S, qn * 64 + fcol);
                        Mma<DT>::step(a, b, acc[kh * 3 + kw]);
                    }
            } else {
#pragma unroll 2
                for (int j = 0; j < 8; ++j) {
                    const int pos = ks * 16 + 2 * j + khalf, oy = pos >> 3, ox = pos & 7;
                    const float a = *(const float*)(smem + pos * ROWB + (qm * 32 + l31) * 4);
#pragma unroll
                    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                        for (int kw = 0; kw < 3; ++kw) {
                            const float b = *(const float*)(xs + ((S * oy + kh) * PW + S * ox + kw) * ROWB + (qn * 32 + l31) * 4);
                            acc[kh * 3 + kw] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[kh * 3 + kw], 0, 0, 0);
                        }
                }
            }
        }
    }
    if (!any) return;                                      // (an empty range, or every chunk outside the clip: nothing to add)
    // ---- kept elements only: row co of the quadrant against column ci of the SAME group ----
    const int cis = qn * 32 + l31;                         // slab-local input channel of this lane
    const int cg = 1 << p.cg_log2;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        float* const Gt = p.G + ((size_t)(kt * 9 + t) * p.C + (size_t)slab * 64) * cg;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int cos = qm * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
            if ((cos >> p.cg_log2) == (cis >> p.cg_log2)) atomicAdd(Gt + (size_t)cos * cg + (cis & (cg - 1)), acc[t][r]);
        }
    }
}

inline int slab_chunks(int dtype) { return dtype == DAT_BF16X3 ? 3 : dtype == DAT_F32 ? 2 : 1; }

// what every grouped entry point accepts (anything else is DAT_ERR_UNSUPPORTED: there is no dense fall-back)
// max_res_mode: the highest residual mode the entry point has (forward: 3 = mask, for DAT_F32 / DAT_BF16; every other one: 0 or 1)
int grouped_check(dat_ctx* ctx, const dat_conv_desc* d, int groups, const char* who, int max_res_mode = 1) {
    DAT_ENFORCE(ctx, d, "%s: null descriptor", who);
    DAT_GRP_UNSUPPORTED(ctx, d->dtype == DAT_F32 || d->dtype == DAT_BF16 || d->dtype == DAT_BF16X3, "%s: bad dtype %d", who, d->dtype);
    DAT_GRP_UNSUPPORTED(ctx, d->dtype != DAT_BF16X3 || DAT_H16_FORMAT == 0,
                        "%s: DAT_BF16X3 needs the bf16 build of the library (this one holds IEEE half in its 16-bit tensors)", who);
    DAT_GRP_UNSUPPORTED(ctx, groups >= 1 && d->Cin > 0 && d->Cin == d->Cout && d->Cin % groups == 0 && d->Cin % 64 == 0,
                        "%s: %d groups must divide Cin %d == Cout %d, a multiple of 64", who, groups, d->Cin, d->Cout);
    const int cg = d->Cin / groups;
    DAT_GRP_UNSUPPORTED(ctx, cg == 4 || cg == 8 || cg == 16 || cg == 32 || cg == 64,
                        "%s: %d channels per group (supported: 4, 8, 16, 32, 64 -- a group must not straddle a 64-channel slab)", who, cg);
    DAT_GRP_UNSUPPORTED(ctx, d->KH == 3 && d->KW == 3 && (d->KT == 1 || d->KT == 3) && d->pad_h == 1 && d->pad_w == 1 && d->pad_t == d->KT / 2,
                        "%s: kernel %dx%dx%d pads %d,%d,%d (supported: 1x3x3 and 3x3x3 with \"same\" padding)", who, d->KT, d->KH, d->KW,
                        d->pad_t, d->pad_h, d->pad_w);
    DAT_GRP_UNSUPPORTED(ctx, d->stride_h == d->stride_w && (d->stride_h == 1 || d->stride_h == 2), "%s: stride %dx%d (supported: 1, 2)", who,
                        d->stride_h, d->stride_w);
    DAT_GRP_UNSUPPORTED(ctx, d->dil_h <= 1 && d->dil_w <= 1, "%s: dilation %dx%d (grouped dilated convs are unsupported)", who, d->dil_h, d->dil_w);
    DAT_GRP_UNSUPPORTED(ctx, d->res_mode == 0 || d->res_mode == 1 || (d->res_mode == 3 && max_res_mode >= 3 && d->dtype != DAT_BF16X3),
                        "%s: res_mode %d (supported: 0, 1%s)", who, d->res_mode,
                        max_res_mode >= 3 ? "; 3 = mask for DAT_F32 / DAT_BF16; 4 = sum + mask has no grouped instantiation" : "");
    return DAT_OK;
}

}  // namespace

extern "C" {

size_t dat_conv3d_grouped_packed_weight_bytes(const dat_conv_desc* d, int groups) {
    if (!d || groups < 1 || d->Cout < 1) return 0;
    return (size_t)d->KT * d->KH * d->KW * slab_chunks(d->dtype) * cout_pad_of(d) * PPITCH;
}

double dat_conv3d_grouped_flops(const dat_conv_desc* d, int groups) {
    if (!d || groups < 1) return 0.0;
    return dat_conv3d_flops(d, d->Cin / groups, d->Cout);
}

int dat_conv3d_grouped_pack_weights(dat_ctx* ctx, dat_stream s, const dat_conv_desc* d, int groups, const float* w, void* packed) {
    DAT_ENFORCE(ctx, d && w && packed, "conv3d_grouped_pack_weights: null argument");
    const int rc = grouped_check(ctx, d, groups, "conv3d_grouped_pack_weights");
    if (rc != DAT_OK) return rc;
    const int ntap = d->KT * d->KH * d->KW, nck = slab_chunks(d->dtype), cp = cout_pad_of(d), cg = d->Cin / groups;
    const size_t total = (size_t)ntap * nck * cp * (d->dtype == DAT_F32 ? 32 : 64);
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
    if (d->dtype == DAT_F32)
        hipLaunchKernelGGL(grouped_pack_kernel<DAT_F32>, dim3(blocks), dim3(256), 0, (hipStream_t)s, w, packed, d->Cout, cg, ntap, cp, nck, 0, 0,
                           (const float*)nullptr);
    else
        hipLaunchKernelGGL(grouped_pack_kernel<DAT_BF16>, dim3(blocks), dim3(256), 0, (hipStream_t)s, w, packed, d->Cout, cg, ntap, cp, nck,
                           d->dtype == DAT_BF16X3 ? 1 : 0, 0, (const float*)nullptr);
    DAT_CHECK_LAUNCH(ctx, "grouped_pack");
    return DAT_OK;
}

int dat_conv3d_grouped_pack_weights_dgrad(dat_ctx* ctx, dat_stream s, const dat_conv_desc* d, int groups, const float* w_fwd,
                                          const float* scale_fwd, void* packed) {
    DAT_ENFORCE(ctx, d && w_fwd && packed, "conv3d_grouped_pack_weights_dgrad: null argument");
    const int rc = grouped_check(ctx, d, groups, "conv3d_grouped_pack_weights_dgrad", 3);
    if (rc != DAT_OK) return rc;
    DAT_GRP_UNSUPPORTED(ctx, d->dtype != DAT_BF16X3, "conv3d_grouped_pack_weights_dgrad: DAT_BF16X3 is an inference mode (no data-gradient pack)");
    DAT_GRP_UNSUPPORTED(ctx, d->stride_h == 1, "conv3d_grouped_pack_weights_dgrad: the data-gradient conv has stride 1 (a stride-2 layer goes "
                        "through dat_zero_insert2x first), got %d", d->stride_h);
    const int ntap = d->KT * d->KH * d->KW, nck = slab_chunks(d->dtype), cp = cout_pad_of(d), cg = d->Cin / groups;
    const size_t total = (size_t)ntap * nck * cp * (d->dtype == DAT_F32 ? 32 : 64);
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
    if (d->dtype == DAT_F32)
        hipLaunchKernelGGL(grouped_pack_kernel<DAT_F32>, dim3(blocks), dim3(256), 0, (hipStream_t)s, w_fwd, packed, d->Cout, cg, ntap, cp, nck, 0, 1,
                           scale_fwd);
    else
        hipLaunchKernelGGL(grouped_pack_kernel<DAT_BF16>, dim3(blocks), dim3(256), 0, (hipStream_t)s, w_fwd, packed, d->Cout, cg, ntap, cp, nck, 0, 1,
                           scale_fwd);
    DAT_CHECK_LAUNCH(ctx, "grouped_pack_dgrad");
    return DAT_OK;
}

// shared by the two weight-gradient entry points: checks + the accumulate launch
static int grouped_wgrad_launch(dat_ctx* ctx, hipStream_t st, const dat_conv_desc* d, int groups, const void* x, const void* g, int g_cstride,
                                float* Gt, const char* who) {
    DAT_ENFORCE(ctx, d && x && g && Gt, "%s: null argument", who);
    const int rc = grouped_check(ctx, d, groups, who, 0);
    if (rc != DAT_OK) return rc;
    DAT_GRP_UNSUPPORTED(ctx, d->dtype != DAT_BF16X3, "%s: DAT_BF16X3 is an inference mode (no weight gradient)", who);
    DAT_GRP_UNSUPPORTED(ctx, d->res_mode == 0, "%s: res_mode %d (a weight gradient has no residual)", who, d->res_mode);
    DAT_ENFORCE(ctx, d->T > 0 && d->frames > 0 && d->frames % d->T == 0, "%s: frames %d not a multiple of T %d", who, d->frames, d->T);
    DAT_ENFORCE(ctx, g_cstride % 8 == 0 && g_cstride >= d->Cout, "%s: g_cstride %d must be a multiple of 8, >= Cout %d", who, g_cstride, d->Cout);
    GWgradParams q;
    memset(&q, 0, sizeof(q));
    q.g = (const char*)g; q.x = (const char*)x; q.G = Gt; q.zeros = (const char*)ctx->zeros;
    q.C = d->Cin; q.g_cs = g_cstride;
    const int cg = d->Cin / groups;
    while ((1 << q.cg_log2) < cg) ++q.cg_log2;
    q.T = d->T; q.H = d->H; q.W = d->W;
    dat_conv3d_out_shape(d, &q.Ho, &q.Wo);
    DAT_ENFORCE(ctx, q.Ho > 0 && q.Wo > 0, "%s: empty output %dx%d", who, q.Ho, q.Wo);
    q.KT = d->KT; q.pt = d->pad_t;
    q.nslab = d->Cin / G_BN; q.frames = d->frames;
    q.tiles_h = (q.Ho + 7) / 8; q.tiles_w = (q.Wo + 7) / 8;
    // (d->out_t0 / out_tn: g is zero outside that window by contract -- its chunks add zeros; the whole clip is reduced)
    const long long nchunks = (long long)d->frames * q.tiles_h * q.tiles_w;
    const long long tiles = (long long)q.nslab * d->KT;
    DAT_ENFORCE(ctx, nchunks < (1ll << 31), "%s: %lld position chunks unsupported", who, nchunks);
    // K split: about two blocks per CU, at least four chunks per block (every block ends in 9 x 64 x cg float atomics)
    long long ks = (2ll * ctx_num_cu(ctx) + tiles - 1) / tiles;
    if (ks > nchunks / 4) ks = nchunks / 4;
    if (ks < 1) ks = 1;
    q.ksplit = (int)ks;
    const int s2 = d->stride_h == 2, f32 = d->dtype == DAT_F32;
    const int pw = 7 * d->stride_h + 3, rowb = f32 ? 256 : 128, rpp = 1024 / rowb;
    const int lds = (64 + pw * pw + rpp - 1) / rpp * rpp * rowb;
    const unsigned nblocks = (unsigned)(tiles * ks);
    ProfBracket prof(ctx, st);
#define DAT_GW_LAUNCH(DT_, S_)                                                              \
    do {                                                                                    \
        auto kern = wgrad_grouped_kernel<DT_, S_>;                                          \
        const int rcl = dat_ensure_lds(ctx, (const void*)kern, 160 * 1024);                 \
        if (rcl != DAT_OK) return rcl;                                                      \
        hipLaunchKernelGGL(kern, dim3(nblocks), dim3(NTHREADS), lds, st, q);                \
    } while (0)
    if (f32 && s2) DAT_GW_LAUNCH(DAT_F32, 2);
    else if (f32) DAT_GW_LAUNCH(DAT_F32, 1);
    else if (s2) DAT_GW_LAUNCH(DAT_BF16, 2);
    else DAT_GW_LAUNCH(DAT_BF16, 1);
#undef DAT_GW_LAUNCH
    DAT_CHECK_LAUNCH(ctx, "wgrad_grouped");
    prof.end(2.0 * d->Cout * cg * d->KT * 9 * (double)d->frames * q.Ho * q.Wo, 64 * 10000 + 2580 + d->dtype);   // ("258": the grouped weight gradient)
    return DAT_OK;
}

size_t dat_conv3d_grouped_wgrad_workspace_bytes(const dat_conv_desc* d, int groups) {
    if (!d || groups < 1 || d->Cout < 1) return 0;
    return (size_t)d->KT * d->KH * d->KW * d->Cout * (d->Cin / groups) * sizeof(float);
}

int dat_conv3d_grouped_wgrad_acc(dat_ctx* ctx, dat_stream s, const dat_conv_desc* d, int groups, const void* x, const void* g, int g_cstride,
                                 float* Gt) {
    return grouped_wgrad_launch(ctx, (hipStream_t)s, d, groups, x, g, g_cstride, Gt, "conv3d_grouped_wgrad_acc");
}

int dat_conv3d_grouped_wgrad(dat_ctx* ctx, dat_stream s, const dat_conv_desc* d, int groups, const void* x, const void* g, int g_cstride,
                             const float* scale, void* workspace, float* dW) {
    DAT_ENFORCE(ctx, d && workspace && dW, "conv3d_grouped_wgrad: null argument");
    const int rc0 = grouped_check(ctx, d, groups, "conv3d_grouped_wgrad", 0);     // (before the memset: nothing is launched for an unsupported call)
    if (rc0 != DAT_OK) return rc0;
    DAT_GRP_UNSUPPORTED(ctx, d->dtype != DAT_BF16X3, "conv3d_grouped_wgrad: DAT_BF16X3 is an inference mode (no weight gradient)");
    hipStream_t st = (hipStream_t)s;
    if (hipMemsetAsync(workspace, 0, dat_conv3d_grouped_wgrad_workspace_bytes(d, groups), st) != hipSuccess)
        DAT_FAIL(ctx, DAT_ERR_LAUNCH, "conv3d_grouped_wgrad: memset failed");
    const int rc = grouped_wgrad_launch(ctx, st, d, groups, x, g, g_cstride, (float*)workspace, "conv3d_grouped_wgrad");
    if (rc != DAT_OK) return rc;
    return launch_wgrad_finish(ctx, st, (const float*)workspace, scale, dW, d->Cout, d->Cin / groups, d->KT * 9);
}

int dat_conv3d_grouped_fwd(dat_ctx* ctx, dat_stream s, const dat_conv_desc* d, int groups, const void* x, const void* w_packed,
                           const float* scale, const float* bias, const void* residual, void* y, void* y_split) {
    DAT_ENFORCE(ctx, d && x && w_packed && y, "conv3d_grouped_fwd: null argument");
    const int rc0 = grouped_check(ctx, d, groups, "conv3d_grouped_fwd", 3);
    if (rc0 != DAT_OK) return rc0;
    const bool x3 = d->dtype == DAT_BF16X3;
    DAT_ENFORCE(ctx, d->T > 0 && d->frames > 0 && d->frames % d->T == 0, "conv3d_grouped_fwd: frames %d not a multiple of T %d", d->frames, d->T);
    DAT_ENFORCE(ctx, d->out_cstride % 8 == 0 && d->out_cstride >= d->Cout, "conv3d_grouped_fwd: out_cstride %d must be a multiple of 8, >= Cout %d",
                d->out_cstride, d->Cout);
    DAT_ENFORCE(ctx, d->res_mode == 0 || residual, "conv3d_grouped_fwd: res_mode %d needs a residual pointer", d->res_mode);
    DAT_ENFORCE(ctx, !y_split || (x3 && d->Cout == d->out_cstride), "conv3d_grouped_fwd: a split output needs DAT_BF16X3 and Cout == out_cstride (got %d / %d)",
                d->Cout, d->out_cstride);
    ConvParams p;
    memset(&p, 0, sizeof(p));
    p.x = (const char*)x; p.w = (const char*)w_packed; p.scale = scale; p.bias = bias;
    p.res = (const char*)residual; p.y = (char*)y; p.y_split = (char*)y_split;
    p.zeros = (const char*)ctx->zeros;
    const int rcw = conv_set_frame_window(ctx, d, p, "conv3d_grouped_fwd");
    if (rcw != DAT_OK) return rcw;
    p.T = d->T; p.H = d->H; p.W = d->W;
    p.Cin = x3 ? 2 * d->Cin : d->Cin;            // (x3: pixel pitch of the hi / lo split tensor)
    p.x3 = x3;
    dat_conv3d_out_shape(d, &p.Ho, &p.Wo);
    DAT_ENFORCE(ctx, p.Ho > 0 && p.Wo > 0, "conv3d_grouped_fwd: empty output %dx%d", p.Ho, p.Wo);
    p.Cout = d->Cout; p.out_cs = d->out_cstride; p.Cout_pad = cout_pad_of(d);
    p.KT = d->KT; p.KH = 3; p.KW = 3; p.sh = p.sw = d->stride_h;
    p.pt = d->pad_t; p.ph = 1; p.pw = 1; p.relu = d->relu; p.res_mode = d->res_mode;
    const TileChoice tc = choose_tile(p.Ho, p.Wo, G_BP_LOG2, p.sh, p.sw, 3, 3);
    p.th_log2 = tc.th_log2; p.tw_log2 = tc.tw_log2;
    const int th = 1 << p.th_log2, tw = 1 << p.tw_log2;
    p.tile_w = tw;
    p.tiles_h = (p.Ho + th - 1) / th;
    p.tiles_w = (p.Wo + tw - 1) / tw;
    p.psh = p.psw = p.sh;
    p.rsh = p.rsw = 1;
    p.PH = th + 2 / p.sh;
    p.PW = tw + 2 / p.sw;
    conv_build_tap_table(p);
    p.pw_magic = conv_pw_magic(p.PW);
    p.n_cchunks = slab_chunks(d->dtype);
    p.ksplit = 1;
    p.nblk_n = d->Cout / G_BN;
    const long long nblocks = (long long)p.frames * p.tiles_h * p.tiles_w * p.nblk_n;
    DAT_ENFORCE(ctx, nblocks > 0 && nblocks < (1ll << 31), "conv3d_grouped_fwd: grid of %lld blocks unsupported", nblocks);
    DAT_ENFORCE(ctx, (long long)p.Ho * p.Wo * p.out_cs * 4 < (1ll << 31) && (long long)p.H * p.W * p.Cin * 4 < (1ll << 31),
                "conv3d_grouped_fwd: one frame of %dx%dx%d exceeds the 2-GB range of the kernel's 32-bit offsets", p.H, p.W, p.Cin);
    p.nblocks = (unsigned)nblocks;
    p.ntiles = (unsigned)(nblocks / p.nblk_n);
    size_t lds = ((size_t)p.PH * p.PW * PPITCH + 1023) & ~(size_t)1023;     // whole 1-KiB DMA pieces
    if (lds < EPI_SLICES_BYTES) lds = EPI_SLICES_BYTES;                     // epilogue staging slices
    DAT_ENFORCE(ctx, lds <= 160 * 1024, "conv3d_grouped_fwd: LDS patch of %zu bytes exceeds 160 KiB (tile %dx%d)", lds, th, tw);
    hipStream_t st = (hipStream_t)s;
    ProfBracket prof(ctx, st);
#define DAT_GRP_LAUNCH(DT_, ODT_, MASK_)                                                               \
    do {                                                                                               \
        auto kern = conv3d_grouped_kernel<DT_, ODT_, MASK_>;                                           \
        const int rc = dat_ensure_lds(ctx, (const void*)kern, 160 * 1024);                              \
        if (rc != DAT_OK) return rc;                                                                   \
        hipLaunchKernelGGL(kern, dim3(p.nblocks), dim3(NTHREADS), lds, st, p);                         \
    } while (0)
    if (x3) DAT_GRP_LAUNCH(DAT_BF16, DAT_F32, false);
    else if (d->res_mode == 3 && d->dtype == DAT_BF16) DAT_GRP_LAUNCH(DAT_BF16, DAT_BF16, true);
    else if (d->res_mode == 3) DAT_GRP_LAUNCH(DAT_F32, DAT_F32, true);
    else if (d->dtype == DAT_BF16) DAT_GRP_LAUNCH(DAT_BF16, DAT_BF16, false);
    else DAT_GRP_LAUNCH(DAT_F32, DAT_F32, false);
#undef DAT_GRP_LAUNCH
    DAT_CHECK_LAUNCH(ctx, "conv3d_grouped");
    prof.end(2.0 * d->Cout * (d->Cin / groups) * d->KT * 9 * (double)p.frames * p.Ho * p.Wo, 64 * 10000 + 2570 + d->dtype);   // ("257 positions": the grouped kernel)
    return DAT_OK;
}

}  // extern "C"
