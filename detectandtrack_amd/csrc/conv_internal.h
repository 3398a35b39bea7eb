// Internal header of the conv translation units (conv3d_igemm.hip: the generic implicit-GEMM kernel, the launch plan of every dense forward
// (conv_plan -> ConvPlan, below) and the launch prologue helpers below; conv_special.hip: the weights-stationary, K-streaming and big-tile
// kernels with their eligibility rules; conv_grouped.hip: the grouped kernel and its own plan; conv_pack.hip: weight packing).  conv_epilogue.h, included below, holds the device pieces the kernels share.  Not part of the C ABI.
#ifndef DAT_CONV_INTERNAL_H
#define DAT_CONV_INTERNAL_H

#include <math.h>
#include <stdlib.h>

#include <type_traits>
#include <utility>

#include "dat_common.h"

namespace dat_conv __attribute__((visibility("hidden"))) {

constexpr int PPITCH = 128; // patch row pitch: one 128-B line per pixel, lane-linear LDS-DMA image, XOR-swizzled
constexpr int NTHREADS = 256;
#ifndef DAT_KT_ROTATE
#define DAT_KT_ROTATE 1
#endif

// 1-KiB pieces of the patch one wave of the unrolled-tap kernels copies (a register of source offsets each): 2-D tiles need
// (16+2)x(16+2) rows = 41 pieces at 256 positions; the linear strips of wide maps (res4: 256 + 2 * 85 + 1 rows) up to 54
constexpr int patch_pieces_per_wave(int ntap, int bp) { return ntap == 10 ? 19 : bp >= 256 ? 14 : 10; }

struct ConvParams {
    const char* x;
    const char* w;
    const float* scale;
    const float* bias;
    const char* res;
    const char* res2;          // res_mode 4: the addend (the other gradient contribution; may be y itself: every element is read and written by one thread)
    char* y;
    char* y_split;              // bf16x3 mode only (ODT fp32): also write the hi / lo bf16 split of y (pixel pitch 2 * out_cs bf16, dat_split_bf16x2's layout) -- the
                                // next conv then needs no split pre-pass; NULL = off
    unsigned long long* dbg;    // DAT_CONV_TRACE builds only: per-phase cycle sums
    unsigned long long* clk;    // profiling only (dat_prof_enable): [0] += shader cycles, [1] += 100-MHz ticks per block
    const char* zeros;          // >= 16 zero bytes (what a halo lane of the patch LDS-DMA fetches)
    int frames, T, H, W, Cin;   // frames = OUTPUT frames (clips * otn)
    int ot0, otn;               // output frames per clip: t in [ot0, ot0 + otn)
    int in_lo, in_hi;           // input frames outside [in_lo, in_hi) of the clip are known to be zero: their temporal taps are skipped
    int Ho, Wo, Cout, out_cs, Cout_pad;
    int KT, KH, KW, sh, sw, pt, ph, pw;
    int relu, res_mode;
    int th_log2, tw_log2;     // output tile = 2^th x 2^tw positions
    int tiles_h, tiles_w;
    int PH, PW;               // patch rows/cols (LDS rows = PH*PW)
    int psh, psw;             // patch sampling step in the input (= conv stride; 1 for the dense stride-2 patch of the NTAP = 10 variant)
    int rsh, rsw;             // patch rows / columns between neighbouring output positions (1; 2 for the dense stride-2 patch)
    int lin_h, lin_w;         // > 0: LINEAR position tiling of small maps (see launch_conv): the real map size; H / W / Ho / Wo then describe a 1 x N strip
    int tile_w;               // output columns between neighbouring tiles
    int lin_zero_row;         // patch row that is all zeros (-1: none): the B fragments of taps that fall outside a map read it
    // spatial tap schedule of one (kt, channel chunk): taps grouped by stride-parity plane, so that every plane is a
    // dense (tile + halo/stride) patch whose rows are read consecutively (stride-2 convs: 4 small patches)
    int tab_n;
    int tab_tap[32];          // kh*KW + kw (weight tap index)
    int tab_rowoff[32];       // LDS row offset of this tap inside the plane patch
    short tab_dy[32], tab_dx[32];  // input offset of the plane's patch cell (0,0) relative to (ih0, iw0)
    unsigned tab_new;         // bit i: entry i starts a new plane (patch reload)
    unsigned pw_magic;        // ceil(2^32 / PW): row / PW == umulhi(row, pw_magic) for row, PW < 2^16; 0 when PW == 1 (2^32 does
                              // not fit: a 1-wide patch of a KW == 1 conv made every row decode to patch row 0)
    int n_cchunks;            // Cin / CK
    int ksplit;               // split-K over the (kt, channel-chunk) sequence; > 1 => fp32 partials to `part`
    float* part;              // [ksplit][frames*Ho*Wo][Cout] fp32 (split-K only)
    int ablate;               // DEBUG (DAT_CONV_ABLATE): 1 skip patch reloads, 4 skip the epilogue, 8 skip patch loads (table-driven loop), 16 no XCD remap
    int nblk_n;               // Cout_pad / BN
    unsigned nblocks;
    unsigned ntiles;          // position tiles (frames x tiles_h x tiles_w)
    int x3;                   // bf16x3 mode: x is the hi / lo split tensor (pixel pitch Cin = 2 x logical channels), channel chunk cc of the K loop reads
                              // source line (cc / 3) * 2 + (cc % 3 == 2); output / residual are fp32 (template parameter ODT)
    int order;                // block order inside an XCD's queue: 0 = (split, cout block) fastest -- the blocks of one tile share its input patch;
                              // 1 = tile fastest -- the resident blocks share ONE (cout block, split) weight slice (layers whose weights exceed the L2)
};

template <int DT> struct Mma;
template <> struct Mma<DAT_BF16> {
    static constexpr int CK = 64;  // channels per 128-B row
    __device__ static __forceinline__ void step(const uint4& a, const uint4& b, f32x16_t& c) {
        c = DAT_MFMA16(a, b, c);
    }
};
template <> struct Mma<DAT_F32> {
    static constexpr int CK = 32;
    __device__ static __forceinline__ void step(const uint4& a, const uint4& b, f32x16_t& c) {
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), c, 0, 0, 0);
    }
};

// residual combine of the fused epilogue: modes 1 / 2 add (Sum shortcut, FPN top-down map); mode 3 MASKS -- out = res > 0 ? v : 0, the
// ReLU backward of the conv's INPUT blob fused into the data-gradient conv (round 3: `res` is the forward input x = relu(...) of the
// conv whose data gradient the launch computes; training.py bwd_Conv)
__device__ __forceinline__ float res_combine(float v, float r, int mode) { return mode == 3 ? (r > 0.f ? v : 0.f) : v + r; }
// mode 4 (round 6): SUM + MASK -- out = m > 0 ? v + old : 0, where `old` is the addend operand (the other contribution to the gradient of a
// residual block's output; it may be the output tensor itself) and `m` the residual operand (that block output y = relu(...)): the data-gradient
// conv of the LAST reader of y finishes the sum and applies y's ReLU backward in one epilogue (dat_conv3d_fwd_sum_mask; training.py bwd_Conv)
__device__ __forceinline__ float res_combine4(float v, float old, float m) { return m > 0.f ? v + old : 0.f; }

}  // namespace dat_conv

#include "conv_epilogue.h"

namespace dat_conv __attribute__((visibility("hidden"))) {

// XOR swizzle of a patch row's eight 16-byte slots (applied on the source side of the LDS-DMA, undone by the B-fragment reads), by MFMA
// shape.  MF = 0 (32x32x16: a 16-lane read group takes 8 + 8 consecutive rows, one k-half): (row >> 1) & 7.  MF = 1 (16x16x32: a read group
// takes 16 consecutive rows, rows 4-11 from the neighbouring k-group of rows 0-3 / 12-15): no XOR of whole slots is conflict-free for every
// first row, so 32-byte slot pairs move by (row >> 1) & 3 and the rows 8 apart that share a pair read its two different halves
// (tests/test_conv_mfma16_cpu.py enumerates the banks).
template <int MF>
__device__ __forceinline__ int patch_swz(int row) { return MF ? ((row >> 1) & 3) << 1 : (row >> 1) & 7; }
// the logical slot the LDS-DMA lane of patch item `it` (row it >> 3, physical slot it & 7) fetches
template <int MF>
__device__ __forceinline__ int patch_src_slot(int it) { const int row = it >> 3; return MF ? (it & 7) ^ patch_swz<1>(row) : (it ^ (row >> 1)) & 7; }
// byte address inside the patch of a lane's B fragment of the first k-slice: k-group kg (lane >> 5 of 2 / lane >> 4 of 4) of patch row `row`;
// the later slices are `^ (ks << 5)` (MF = 0, K = 16 each) / `^ (s << 6)` (MF = 1, K = 32 each)
template <int MF>
__device__ __forceinline__ unsigned patch_frag_addr(int row, int kg) {
    if (MF) return (unsigned)(row * PPITCH) + (unsigned)((kg ^ patch_swz<1>(row)) << 4);
    const int g = (row >> 1) & 7;
    return (unsigned)(row * PPITCH) + (unsigned)(((kg ^ (g & 1)) << 4) | ((g >> 1) << 5));
}

// compile-time index sequence for the hand-scheduled loops (`#pragma unroll` is refused for bodies of this size, and immediates /
// register-ring slots need constant indices)
template <int... I, class F>
__device__ __forceinline__ void static_for(std::integer_sequence<int, I...>, F&& f) {
    (f(std::integral_constant<int, I>{}), ...);
}


inline int cout_pad_of(const dat_conv_desc* d) {
    const int bn = d->Cout <= 64 ? 64 : 128;
    return (d->Cout + bn - 1) / bn * bn;
}

// spatial dilation of a descriptor: 0 and 1 both mean "not dilated", and a 1x1 spatial kernel has nothing to dilate.  Every kernel's
// *_eligible predicate that has spatial taps asks this and declines d > 1; only the generic kernel's host-built patch geometry knows it.
inline int conv_dilation(const dat_conv_desc* d) { return (d->KH > 1 || d->KW > 1) && d->dil_h > 1 ? d->dil_h : 1; }
// what every dense entry point that takes a descriptor refuses about the dilation fields (NULL: nothing), for the caller's error text
inline const char* conv_dilation_refusal(const dat_conv_desc* d) {
    if (d->KH == 1 && d->KW == 1) return nullptr;
    if (d->dil_h < 0 || d->dil_w < 0) return "negative dilation";
    if ((d->dil_h > 1 ? d->dil_h : 1) != (d->dil_w > 1 ? d->dil_w : 1)) return "dil_h != dil_w is unsupported (spatial dilation is equal in H and W)";
    if (d->dil_h > 1 && (d->stride_h != 1 || d->stride_w != 1)) return "dilation with a spatial stride > 1 is unsupported";
    return nullptr;
}

// ---- launch prologue shared by launch_conv and dat_conv3d_grouped_fwd (conv3d_igemm.hip) ----
struct TileChoice {
    int th_log2, tw_log2;
};
// the 2^a x 2^b output tile (a + b = bp_log2) that wastes the fewest output positions, tie -> squarer patch
TileChoice choose_tile(int Ho, int Wo, int bp_log2, int sh, int sw, int KH, int KW);
// spatial tap schedule in stride-parity plane order (tab_*, tab_new, tab_n) from KH / KW / sh / sw / PW; KH * KW <= 32
void conv_build_tap_table(ConvParams& p);
// ConvParams::pw_magic
inline unsigned conv_pw_magic(int PW) { return PW == 1 ? 0u : (unsigned)((0x100000000ull + (unsigned)PW - 1) / (unsigned)PW); }
// in_lo / in_hi / ot0 / otn / frames of `p` from the descriptor's frame windows; `who` names the entry point in the error text
int conv_set_frame_window(dat_ctx* ctx, const dat_conv_desc* d, ConvParams& p, const char* who);

// per-launch timing (dat_prof_enable): takes the context's next event pair and records the first one, unless the stream is being
// captured -- an event recorded there becomes a graph node, and timing it later fails with hipErrorInvalidHandle, a sticky error the
// host framework then reports at an unrelated call.  end() records the second event with the launch's flops and kernel tag.
struct ProfBracket {
    dat_ctx* ctx;
    hipStream_t st;
    hipEvent_t e1 = nullptr;
    ProfBracket(dat_ctx* ctx_, hipStream_t st_) : ctx(ctx_), st(st_) {
        hipStreamCaptureStatus cap_st = hipStreamCaptureStatusNone;
        if (ctx->prof_enabled && ctx->prof_n < ctx->prof_cap && hipStreamIsCapturing(st, &cap_st) == hipSuccess &&
            cap_st == hipStreamCaptureStatusNone) {
            e1 = ctx->prof_ev[2 * ctx->prof_n + 1];
            hipEventRecord(ctx->prof_ev[2 * ctx->prof_n], st);
        }
    }
    void end(double flops, int tag) {
        if (!e1) return;
        hipEventRecord(e1, st);
        ctx->prof_flops[ctx->prof_n] = flops;
        ctx->prof_tag[ctx->prof_n] = tag;
        ctx->prof_n++;
    }
};

// What a dense conv launch does with a descriptor, and nothing about its tensors (the C ABI's dat_conv_plan: dat_conv3d_plan shows it).
// conv_plan (conv3d_igemm.hip) derives it once per launch from the context's knobs, the CU count and the descriptor; the launchers below
// take their tile, split-K factor and grid from it.
typedef dat_conv_plan ConvPlan;

// conv_special.hip: what each special kernel assumes about a layer (its grid rule included: `num_cu` compute units), the tile / grid
// it would run, and its launcher
int ctx_num_cu(dat_ctx* ctx);
bool ws64_eligible(const dat_ctx* ctx, const dat_conv_desc* d);
int ws64_tile_twl(const dat_ctx* ctx, int num_cu, const ConvParams& p, long long* ntiles);
long long ws64_grid(const dat_ctx* ctx, int num_cu, long long ntiles);
int launch_ws64(dat_ctx* ctx, hipStream_t st, const ConvParams& cp, const ConvPlan& plan);
bool pw256_eligible(const dat_ctx* ctx, const dat_conv_desc* d);
long long pw256_grid(const dat_ctx* ctx, int num_cu, const ConvParams& cp);
int launch_pw256(dat_ctx* ctx, hipStream_t st, const ConvParams& cp, const ConvPlan& plan);
bool pwlw_eligible(const dat_ctx* ctx, int num_cu, const dat_conv_desc* d);
long long pwlw_grid(const dat_ctx* ctx, int num_cu, const ConvParams& cp);
int launch_pwlw(dat_ctx* ctx, hipStream_t st, const ConvParams& cp, const ConvPlan& plan);
bool pwks_eligible(const dat_ctx* ctx, int num_cu, const dat_conv_desc* d);
bool tks_eligible(const dat_ctx* ctx, int num_cu, const dat_conv_desc* d);
long long ks_grid(const ConvParams& cp);
int launch_pwks(dat_ctx* ctx, hipStream_t st, const ConvParams& cp, const ConvPlan& plan);
int launch_tks(dat_ctx* ctx, hipStream_t st, const ConvParams& cp, const ConvPlan& plan);
bool bt_eligible(const dat_ctx* ctx, const dat_conv_desc* d);
int bt_tile_twl(const ConvParams& p, long long* nblocks);
int launch_bt(dat_ctx* ctx, hipStream_t st, ConvParams& p, const ConvPlan& plan);

// train_ops.hip: dW[co][ci][tap] = scale[co] * Gt[tap][co][ci] (wgrad_finish_kernel; scale NULL = 1)
int launch_wgrad_finish(dat_ctx* ctx, hipStream_t st, const float* Gt, const float* scale, float* dW, int Cout, int Cin, int ntaps);

}  // namespace dat_conv

#endif
