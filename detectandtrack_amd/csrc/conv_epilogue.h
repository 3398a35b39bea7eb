// Include only from conv_internal.h (it uses res_combine / res_combine4 declared there, and bf2f / f2bf2 / f32x16_t of dat_common.h).
// The pieces the implicit-GEMM, special and grouped conv kernels share around their own main loops: the XCD-aware block map and the
// LDS-transposed fused epilogue.  DESIGN.md section 3.9.
//
// The MFMA result layout gives a lane 4 channels of ONE position (register r -> channel (r&3) + 8*(r>>2) + 4*(lane>>5)), i.e. 8-byte
// pieces 512+ bytes apart: written directly, every store instruction touched 32-64 different lines and a 256x128 tile took ~47k cycles
// (1x1 convs spent 80 % of their time here).  Each wave therefore transposes 32 positions at a time through its own fp32 LDS slice
// (row pitch = channels * 4 + 16 B: conflict-free b128 writes) and reads it back position-major, 16 B of output per lane, so one store
// instruction covers whole channel runs.  A kernel supplies what differs: its position decode, how it prefetches the residual rows,
// its scale / bias convention for channels past Cout, and any split-K partial path.  The helpers are the steps in between, in the
// order every kernel applies them: epi_stage | epi_stage16 (the accumulator layout of the 16x16x32 MFMA shape), (wave barrier), epi_load,
// epi_affine, epi_residual | epi_residual4, epi_relu, epi_store.
#ifndef DAT_CONV_EPILOGUE_H
#define DAT_CONV_EPILOGUE_H

namespace dat_conv __attribute__((visibility("hidden"))) {

constexpr int EPI_PITCH = 64 * 4 + 16;   // slice row of the kernels that transpose 64 channels at a time
constexpr int EPI_SLICES_BYTES = 4 * 32 * EPI_PITCH;   // the four per-wave slices of a 256-thread block

// XCD-aware block map (bijective for any grid size): hardware block b runs on XCD b % 8; the result numbers the blocks so that
// consecutive LOGICAL ids -- the channel blocks of one tile, neighbouring tiles -- sit in one XCD's queue and share its L2
__device__ __forceinline__ unsigned xcd_block_map(unsigned bid, unsigned nblocks) {
    const unsigned nx = 8, q = nblocks / nx, r = nblocks % nx;
    const unsigned xcd = bid % nx, k = bid / nx;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
}

// accumulators of 32-row block i of one 32-position group -> LDS [position `row` = lane & 31][channel] fp32
template <int PITCH = EPI_PITCH>
__device__ __forceinline__ void epi_stage(char* est, int row, int khalf, int i, const f32x16_t& acc) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
        *(float4*)(est + row * PITCH + (i * 32 + g * 8 + khalf * 4) * 4) = make_float4(acc[g * 4 + 0], acc[g * 4 + 1], acc[g * 4 + 2], acc[g * 4 + 3]);
}

// the same staging step for the 16x16x32 MFMA shape, whose accumulator tile holds column (position) lane & 15 and rows (channels)
// (lane >> 4) * 4 + register: 16-row block i16 of the 64 channels, 16-position half jl of the 32-position group -> the same LDS image,
// so everything after the transpose is shared
template <int PITCH = EPI_PITCH>
__device__ __forceinline__ void epi_stage16(char* est, int lane, int i16, int jl, const f32x4_t& acc) {
    *(float4*)(est + (jl * 16 + (lane & 15)) * PITCH + (i16 * 16 + (lane >> 4) * 4) * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

// position-major read back: CPL channels from channel sl_c of position pl
template <int CPL, int PITCH = EPI_PITCH>
__device__ __forceinline__ void epi_load(const char* est, int pl, int sl_c, float (&v)[CPL]) {
#pragma unroll
    for (int e4 = 0; e4 < CPL / 4; ++e4) {
        const float4 t = *(const float4*)(est + pl * PITCH + sl_c * 4 + e4 * 16);
        v[e4 * 4 + 0] = t.x; v[e4 * 4 + 1] = t.y; v[e4 * 4 + 2] = t.z; v[e4 * 4 + 3] = t.w;
    }
}

template <int CPL>
__device__ __forceinline__ void epi_affine(float (&v)[CPL], const float (&sc)[CPL], const float (&bi)[CPL]) {
#pragma unroll
    for (int e = 0; e < CPL; ++e) v[e] = v[e] * sc[e] + bi[e];
}

// residual combine (res_combine: modes 1 / 2 sum, 3 mask) with a prefetched 16-byte row piece of ODT elements.  (Written pair by pair
// and not as one loop over the elements: the compiler then keeps the packed fp32 adds)
template <int ODT, int CPL>
__device__ __forceinline__ void epi_residual(float (&v)[CPL], const uint4& r, int mode) {
    if (ODT == DAT_BF16) {
        const uint32_t ru[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int e2 = 0; e2 < CPL / 2; ++e2) {
            v[2 * e2] = res_combine(v[2 * e2], bf2f((uint16_t)(ru[e2 % 4] & 0xffff)), mode);
            v[2 * e2 + 1] = res_combine(v[2 * e2 + 1], bf2f((uint16_t)(ru[e2 % 4] >> 16)), mode);
        }
    } else {
        v[0] = res_combine(v[0], __uint_as_float(r.x), mode); v[1] = res_combine(v[1], __uint_as_float(r.y), mode);
        v[2] = res_combine(v[2], __uint_as_float(r.z), mode); v[3] = res_combine(v[3], __uint_as_float(r.w), mode);
    }
}

// mode 4 (res_combine4: sum with `addend`, masked by `mask`), 16-bit rows
template <int ODT, int CPL>
__device__ __forceinline__ void epi_residual4(float (&v)[CPL], const uint4& addend, const uint4& mask) {
    static_assert(ODT == DAT_BF16, "the kernels that prefetch both rows of mode 4 are 16-bit ones");
    const uint32_t au[4] = {addend.x, addend.y, addend.z, addend.w}, mu[4] = {mask.x, mask.y, mask.z, mask.w};
#pragma unroll
    for (int e2 = 0; e2 < CPL / 2; ++e2) {
        v[2 * e2] = res_combine4(v[2 * e2], bf2f((uint16_t)(au[e2 % 4] & 0xffff)), bf2f((uint16_t)(mu[e2 % 4] & 0xffff)));
        v[2 * e2 + 1] = res_combine4(v[2 * e2 + 1], bf2f((uint16_t)(au[e2 % 4] >> 16)), bf2f((uint16_t)(mu[e2 % 4] >> 16)));
    }
}

template <int CPL>
__device__ __forceinline__ void epi_relu(float (&v)[CPL], int relu) {
    if (relu) {
#pragma unroll
        for (int e = 0; e < CPL; ++e) v[e] = fmaxf(v[e], 0.f);
    }
}

// the 16 bytes of output a lane holds: 8 packed 16-bit values or 4 fp32
template <int ODT, int CPL>
__device__ __forceinline__ void epi_store(char* yp, const float (&v)[CPL]) {
    static_assert(CPL == (ODT == DAT_BF16 ? 8 : 4), "a lane stores 16 bytes");
    if (ODT == DAT_BF16) *(uint4*)yp = make_uint4(f2bf2(v[0], v[1]), f2bf2(v[2], v[3]), f2bf2(v[4 % CPL], v[5 % CPL]), f2bf2(v[6 % CPL], v[7 % CPL]));
    else *(float4*)yp = make_float4(v[0], v[1], v[2], v[3]);
}

// bf16x3 mode: four fp32 values as hi / lo bf16 halves for the next bf16x3 conv, bit-identical to dat_split_bf16x2 of the stored values.
// `sp` = the hi line of the pixel's 64-channel chunk (line 2q of chunk q) at these 4 channels; the lo line follows 128 bytes later
__device__ __forceinline__ void split_hi_lo_store(char* sp, const float* v) {
    const uint32_t h0 = f2bf2(v[0], v[1]), h1 = f2bf2(v[2], v[3]);
    const uint32_t l0 = f2bf2(v[0] - __uint_as_float(h0 << 16), v[1] - __uint_as_float(h0 & 0xffff0000u));
    const uint32_t l1 = f2bf2(v[2] - __uint_as_float(h1 << 16), v[3] - __uint_as_float(h1 & 0xffff0000u));
    *(uint2*)sp = make_uint2(h0, h1);
    *(uint2*)(sp + 128) = make_uint2(l0, l1);
}

}  // namespace dat_conv

#endif
