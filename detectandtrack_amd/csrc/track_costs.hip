// Tracker appearance cost on the device (gfx950): the two kernels around the ResNet-18 trunk of TRACKING.DISTANCE_METRICS 'cnn-cosdist'
// (reference lib/core/tracking_engine.py:132-155, lib/utils/pytorch_cnn_features.py).
//
// dat_crop_resize_patches: every box of a frame is cut out of the uploaded uint8 BGR frame, resized to out x out with the 8-bit bilinear
// rule of utils/image.resize_bilinear_u8 (integer arithmetic: 11-bit weights, int32 horizontal pass, (.. + 2^21) >> 22 vertical pass),
// turned RGB / CHW and normalised (v / 255 - mean) / std in double, rounded once to fp32 -- the `data` blob [n, 3, 1, out, out] the fused
// stem reads.  Bit-identical to the host restatement: the source coordinate is formed in double in NumPy's operation order (this file is
// compiled with -ffp-contract=off: a fused (d + 0.5) * step - 0.5 would round differently).
//
// dat_cosine_cost: C[i][j] = 1 - a_i . b_j / (|a_i| |b_j|) for feature rows of up to a few 100 k elements.  Blocks own chunks of the
// feature axis; a block writes its partial Gram slab [n][m] and the partial squared norms of its chunk to the workspace (MFMA for the
// 16-bit build format, the f32 MFMA for fp32), a second small kernel sums the slabs in chunk order and finishes.  No float atomics: the
// result depends on (n, m, D) only, run after run.
#include "dat_common.h"

namespace {

// ---- crop + 8-bit resize + normalise -------------------------------------------------------------------------------------------------
constexpr int CROP_MAX = 128;      // boxes per launch (their ranges travel as kernel arguments)

struct CropParams {
    const uint8_t* frame;   // [h][w][3] BGR
    float* data;            // [n][3][1][out][out], RGB planes
    int h, w, out, box0;
    double mean[3], stdv[3];
    int ranges[CROP_MAX][4];   // x0, x1, y0, y1 (resolved slices: [x0, x1) x [y0, y1) inside the frame; x1 <= x0 or y1 <= y0: empty)
};

// destination index d of an axis resized n_src -> n_dst: the two source indices and their 11-bit weights (cv::resize's 8-bit INTER_LINEAR
// tables).  snap (x): positions outside the image read the border pixel with weights (2048, 0); else (y): weights kept, indices clamped.
__device__ __forceinline__ void u8_axis(int d, int n_src, int n_dst, bool snap, int* i0, int* i1, int* w0, int* w1) {
    const double step = 1.0 / ((double)n_dst / (double)n_src);
    const float f = (float)(((double)d + 0.5) * step - 0.5);
    const float fl = floorf(f);
    int s = (int)fl;
    float t = f - fl;
    if (snap) {
        if (s < 0 || s >= n_src - 1) t = 0.f;
        s = min(max(s, 0), n_src - 1);
        *i0 = s;
        *i1 = min(s + 1, n_src - 1);
    } else {
        *i0 = min(max(s, 0), n_src - 1);
        *i1 = min(max(s + 1, 0), n_src - 1);
    }
    *w0 = (int)rintf((1.f - t) * 2048.f);       // each weight rounded on its own, half to even (saturate_cast<short>)
    *w1 = (int)rintf(t * 2048.f);
}

__global__ __launch_bounds__(256) void crop_resize_kernel(const CropParams p) {
    const int b = blockIdx.y;
    const int px = blockIdx.x * 256 + threadIdx.x;
    const int plane = p.out * p.out;
    if (px >= plane) return;
    const int oy = px / p.out, ox = px - oy * p.out;
    const int x0 = p.ranges[b][0], x1 = p.ranges[b][1], y0 = p.ranges[b][2], y1 = p.ranges[b][3];
    const int sw = x1 - x0, sh = y1 - y0;
    int v[3] = {0, 0, 0};       // BGR; an empty crop is an all-zero image
    if (sw > 0 && sh > 0) {
        int ix0, ix1, wx0, wx1, iy0, iy1, wy0, wy1;
        u8_axis(ox, sw, p.out, true, &ix0, &ix1, &wx0, &wx1);
        u8_axis(oy, sh, p.out, false, &iy0, &iy1, &wy0, &wy1);
        const uint8_t* r0 = p.frame + ((size_t)(y0 + iy0) * p.w + x0) * 3;
        const uint8_t* r1 = p.frame + ((size_t)(y0 + iy1) * p.w + x0) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int top = (int)r0[ix0 * 3 + c] * wx0 + (int)r0[ix1 * 3 + c] * wx1;     // horizontal pass, int32
            const int bot = (int)r1[ix0 * 3 + c] * wx0 + (int)r1[ix1 * 3 + c] * wx1;
            const int q = (wy0 * top + wy1 * bot + (1 << 21)) >> 22;                     // <= 2049 * 2049 * 255 + 2^21 < 2^31
            v[c] = min(max(q, 0), 255);
        }
    }
    float* o = p.data + (size_t)(p.box0 + b) * 3 * plane + px;
#pragma unroll
    for (int c = 0; c < 3; ++c)       // plane c of the blob is R, G, B = BGR channel 2 - c
        o[(size_t)c * plane] = (float)(((double)v[2 - c] / 255.0 - p.mean[c]) / p.stdv[c]);
}

// ---- cosine cost ----------------------------------------------------------------------------------------------------------------------
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

constexpr int COS_TILE = 128;          // rows of fa x rows of fb per block: four waves, 64 x 64 each (4 x 4 MFMA tiles of 16 x 16)
constexpr int COS_MAX_ROWS = 1024;
constexpr int COS_CHUNK_MIN = 256, COS_CHUNKS = 128;
constexpr size_t COS_SLAB_BYTES = (size_t)32 << 20;     // the Gram slabs of all chunks stay below this

struct CosPlan {
    int kc, nch;    // feature elements per chunk (a multiple of 64), chunks
};

static CosPlan cos_plan(int n, int m, long long D) {
    long long want = COS_CHUNKS;
    const long long cap = (long long)(COS_SLAB_BYTES / ((size_t)n * m * 4));
    if (want > cap) want = cap < 1 ? 1 : cap;
    long long kc = cdiv_ll(cdiv_ll(D, want), 64) * 64;
    if (kc < COS_CHUNK_MIN) kc = COS_CHUNK_MIN;
    CosPlan pl;
    pl.kc = (int)kc;
    pl.nch = (int)cdiv_ll(D, kc);
    return pl;
}

static size_t cos_ws_bytes(int n, int m, long long D) {
    const CosPlan pl = cos_plan(n, m, D);
    return (size_t)pl.nch * ((size_t)n * m + n + m) * sizeof(float);
}

struct CosParams {
    const void* fa;     // [n][ld]
    const void* fb;     // [m][ld]
    float* gram;        // [nch][n][m]
    float* na;          // [nch][n]
    float* nb;          // [nch][m]
    int n, m, kc, nch, vec;
    long long D, ld;
};

template <int DT> struct CosFrag;
// 16-bit build format: one 16 x 16 x 32 MFMA per fragment pair; a lane holds 8 consecutive elements of row (lane & 15) at k part (lane >> 4)
template <> struct CosFrag<DAT_BF16> {
    static constexpr int EPL = 8;
    typedef u32x4_t frag;
    __device__ static __forceinline__ frag load(const void* base, long long off, long long k, long long k1, bool live, int vec) {
        frag f = {0u, 0u, 0u, 0u};
        if (!live) return f;
        const uint16_t* src = (const uint16_t*)base + off + k;
        if (vec && k + EPL <= k1) return *(const frag*)src;         // 16 bytes
        uint16_t e[EPL];
#pragma unroll
        for (int j = 0; j < EPL; ++j) e[j] = k + j < k1 ? src[j] : (uint16_t)0;
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = (uint32_t)e[2 * j] | ((uint32_t)e[2 * j + 1] << 16);
        return f;
    }
    __device__ static __forceinline__ float sumsq(const frag& f) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float lo = bf2f((uint16_t)(f[j] & 0xffffu)), hi = bf2f((uint16_t)(f[j] >> 16));
            s += lo * lo;
            s += hi * hi;
        }
        return s;
    }
    __device__ static __forceinline__ f32x4_t mma(const frag& a, const frag& b, f32x4_t c) { return DAT_MFMA16K32(a, b, c); }
};
// fp32: four 16 x 16 x 4 MFMAs per fragment pair; a lane holds 4 consecutive elements
template <> struct CosFrag<DAT_F32> {
    static constexpr int EPL = 4;
    typedef f32x4_t frag;
    __device__ static __forceinline__ frag load(const void* base, long long off, long long k, long long k1, bool live, int vec) {
        frag f = {0.f, 0.f, 0.f, 0.f};
        if (!live) return f;
        const float* src = (const float*)base + off + k;
        if (vec && k + EPL <= k1) return *(const frag*)src;         // 16 bytes
#pragma unroll
        for (int j = 0; j < EPL; ++j) f[j] = k + j < k1 ? src[j] : 0.f;
        return f;
    }
    __device__ static __forceinline__ float sumsq(const frag& f) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) s += f[j] * f[j];
        return s;
    }
    __device__ static __forceinline__ f32x4_t mma(const frag& a, const frag& b, f32x4_t c) {
#pragma unroll
        for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], c, 0, 0, 0);
        return c;
    }
};

// grid (chunk, 128-row tile of fa, 128-row tile of fb).  Both operands of an MFMA map lane -> k the same way, so the order of k inside a
// step does not matter; the result tile has its column on (lane & 15) and rows 4 * (lane >> 4) + reg.
template <int DT>
__global__ __launch_bounds__(256) void cosine_partial_kernel(const CosParams p) {
    typedef CosFrag<DT> F;
    constexpr int KSTEP = 4 * F::EPL;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int row0 = blockIdx.y * COS_TILE + (wave >> 1) * 64, col0 = blockIdx.z * COS_TILE + (wave & 1) * 64;
    const int chunk = blockIdx.x;
    const long long k0 = (long long)chunk * p.kc, k1 = min(k0 + (long long)p.kc, p.D);
    const int rt = min(max((p.n - row0 + 15) / 16, 0), 4), ct = min(max((p.m - col0 + 15) / 16, 0), 4);    // live 16-row tiles
    if (rt == 0 || ct == 0) return;                    // (wave-uniform; the waves that own the norms sit at col0 = 0 / row0 = 0: ct, rt > 0)
    const bool norm_a = blockIdx.z == 0 && (wave & 1) == 0, norm_b = blockIdx.y == 0 && (wave >> 1) == 0;
    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float sa[4] = {0.f, 0.f, 0.f, 0.f}, sb[4] = {0.f, 0.f, 0.f, 0.f};
    for (long long k = k0; k < k1; k += KSTEP) {
        const long long kk = k + q * F::EPL;
        typename F::frag a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = row0 + 16 * i + r;
            a[i] = F::load(p.fa, (long long)row * p.ld, kk, k1, i < rt && row < p.n && kk < k1, p.vec);
            const int col = col0 + 16 * i + r;
            b[i] = F::load(p.fb, (long long)col * p.ld, kk, k1, i < ct && col < p.m && kk < k1, p.vec);
        }
        if (norm_a) {
#pragma unroll
            for (int i = 0; i < 4; ++i) sa[i] += F::sumsq(a[i]);
        }
        if (norm_b) {
#pragma unroll
            for (int i = 0; i < 4; ++i) sb[i] += F::sumsq(b[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i < rt && j < ct) acc[i][j] = F::mma(a[i], b[j], acc[i][j]);
    }
    float* g = p.gram + (size_t)chunk * p.n * p.m;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = col0 + 16 * j + r;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = row0 + 16 * i + 4 * q + e;
                if (i < rt && j < ct && row < p.n && col < p.m) g[(size_t)row * p.m + col] = acc[i][j][e];
            }
        }
    // a row's squared norm over the chunk: its four k parts sit on lanes r, r + 16, r + 32, r + 48
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float va = sa[i], vb = sb[i];
        va += __shfl_xor(va, 16);
        va += __shfl_xor(va, 32);
        vb += __shfl_xor(vb, 16);
        vb += __shfl_xor(vb, 32);
        const int row = row0 + 16 * i + r, col = col0 + 16 * i + r;
        if (norm_a && q == 0 && i < rt && row < p.n) p.na[(size_t)chunk * p.n + row] = va;
        if (norm_b && q == 0 && i < ct && col < p.m) p.nb[(size_t)chunk * p.m + col] = vb;
    }
}

// one thread per (i, j): the chunks' partial sums added in chunk order, then 1 - d / sqrt(|a|^2 |b|^2); a zero norm gives distance 1
__global__ __launch_bounds__(256) void cosine_finish_kernel(const float* gram, const float* na, const float* nb, int n, int m, int nch, float* cost) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)n * m) return;
    const int i = (int)(t / m), j = (int)(t - (long long)i * m);
    float d = 0.f, a = 0.f, b = 0.f;
    for (int c = 0; c < nch; ++c) {
        d += gram[(size_t)c * n * m + t];
        a += na[(size_t)c * n + i];
        b += nb[(size_t)c * m + j];
    }
    cost[t] = (a == 0.f || b == 0.f) ? 1.f : 1.f - d / sqrtf(a * b);
}

}  // namespace

extern "C" {

int dat_crop_resize_patches(dat_ctx* ctx, dat_stream s, const unsigned char* frame, int h, int w, const int* ranges, int n, int out,
                            const double* mean, const double* stdv, float* data) {
    DAT_ENFORCE(ctx, n >= 0, "crop_resize_patches: %d boxes", n);
    DAT_ENFORCE(ctx, out >= 1 && out <= 4096, "crop_resize_patches: output size %d (1 .. 4096)", out);
    DAT_ENFORCE(ctx, h >= 1 && w >= 1 && (long long)h * w < (1ll << 30), "crop_resize_patches: frame %d x %d", h, w);
    if (n == 0) return DAT_OK;
    DAT_ENFORCE(ctx, frame && ranges && mean && stdv && data, "crop_resize_patches: null argument");
    for (int c = 0; c < 3; ++c) DAT_ENFORCE(ctx, stdv[c] != 0.0, "crop_resize_patches: std[%d] is zero", c);
    for (int i = 0; i < n; ++i) {
        const int* q = ranges + 4 * i;
        DAT_ENFORCE(ctx, q[0] >= 0 && q[0] <= w && q[1] >= 0 && q[1] <= w && q[2] >= 0 && q[2] <= h && q[3] >= 0 && q[3] <= h,
                    "crop_resize_patches: range %d [%d, %d) x [%d, %d) lies outside the %d x %d frame", i, q[0], q[1], q[2], q[3], w, h);
    }
    CropParams p;
    p.frame = frame; p.data = data; p.h = h; p.w = w; p.out = out;
    for (int c = 0; c < 3; ++c) { p.mean[c] = mean[c]; p.stdv[c] = stdv[c]; }
    for (int b0 = 0; b0 < n; b0 += CROP_MAX) {         // one launch per 128 boxes: a frame's boxes in one
        const int cnt = n - b0 < CROP_MAX ? n - b0 : CROP_MAX;
        p.box0 = b0;
        memcpy(p.ranges, ranges + 4 * (size_t)b0, sizeof(int) * 4 * cnt);
        hipLaunchKernelGGL(crop_resize_kernel, dim3((unsigned)((out * out + 255) / 256), (unsigned)cnt), dim3(256), 0, (hipStream_t)s, p);
    }
    DAT_CHECK_LAUNCH(ctx, "crop_resize_patches");
    return DAT_OK;
}

size_t dat_cosine_cost_workspace_bytes(int n, int m, long long D) {
    if (n < 1 || m < 1 || n > COS_MAX_ROWS || m > COS_MAX_ROWS || D < 1) return 0;
    return cos_ws_bytes(n, m, D);
}

int dat_cosine_cost(dat_ctx* ctx, dat_stream s, int dtype, const void* fa, int n, const void* fb, int m, long long D, long long ld,
                    float* cost, void* ws, size_t ws_bytes) {
    DAT_ENFORCE(ctx, dtype == DAT_F32 || dtype == DAT_BF16, "cosine_cost: dtype %d", dtype);
    DAT_ENFORCE(ctx, n >= 0 && m >= 0 && n <= COS_MAX_ROWS && m <= COS_MAX_ROWS, "cosine_cost: %d x %d rows (at most %d each)", n, m,
                COS_MAX_ROWS);
    DAT_ENFORCE(ctx, D >= 1 && D <= ld && ld < (1ll << 40), "cosine_cost: %lld features at row stride %lld", D, ld);
    if (n == 0 || m == 0) return DAT_OK;
    DAT_ENFORCE(ctx, fa && fb && cost && ws, "cosine_cost: null argument");
    DAT_ENFORCE(ctx, ws_bytes >= cos_ws_bytes(n, m, D), "cosine_cost: workspace of %zu bytes, %zu needed", ws_bytes, cos_ws_bytes(n, m, D));
    const CosPlan pl = cos_plan(n, m, D);
    CosParams p;
    p.fa = fa; p.fb = fb; p.n = n; p.m = m; p.kc = pl.kc; p.nch = pl.nch; p.D = D; p.ld = ld;
    p.gram = (float*)ws;
    p.na = p.gram + (size_t)pl.nch * n * m;
    p.nb = p.na + (size_t)pl.nch * n;
    // 16-byte operand loads need 16-byte aligned rows (chunks start at multiples of 64 elements)
    const int epv = 16 / dat_esize(dtype);
    p.vec = ld % epv == 0 && ((uintptr_t)fa & 15) == 0 && ((uintptr_t)fb & 15) == 0;
    const dim3 grid((unsigned)pl.nch, (unsigned)((n + COS_TILE - 1) / COS_TILE), (unsigned)((m + COS_TILE - 1) / COS_TILE));
    if (dtype == DAT_BF16)
        hipLaunchKernelGGL(cosine_partial_kernel<DAT_BF16>, grid, dim3(256), 0, (hipStream_t)s, p);
    else
        hipLaunchKernelGGL(cosine_partial_kernel<DAT_F32>, grid, dim3(256), 0, (hipStream_t)s, p);
    hipLaunchKernelGGL(cosine_finish_kernel, dim3((unsigned)(((long long)n * m + 255) / 256)), dim3(256), 0, (hipStream_t)s,
                       (const float*)p.gram, (const float*)p.na, (const float*)p.nb, n, m, pl.nch, cost);
    DAT_CHECK_LAUNCH(ctx, "cosine_cost");
    return DAT_OK;
}

}  // extern "C"
