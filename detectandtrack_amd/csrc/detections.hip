// Detection post-processing on the device (gfx950): the reference's host glue between `model.net` and `model.keypoint_net`.
//
// Replaces, without a host round trip,
//   lib/core/test.py:215-252  im_detect_bbox tail: rois / im_scale, bbox_transform with MODEL.BBOX_REG_WEIGHTS
//                             (lib/utils/boxes.py:141-202), clip_tiled_boxes to the image (:243-253);
//   lib/core/test.py:750-806  box_results_with_nms_and_limit: per class score > TEST.SCORE_THRESH, NMS (TEST.NMS),
//                             then TEST.DETECTIONS_PER_IM over all classes (scores >= the D-th best);
//   lib/core/test.py:78-123   _get_rois_blob: the kept boxes * im_scale with a leading level column = `keypoint_rois`.
// The reference fetches rois / cls_prob / bbox_pred to the host (a device sync per clip), loops over classes in NumPy, calls
// the NMS, and feeds `keypoint_rois` back.  Here the chain is: one select+decode kernel and one NMS per foreground class (or, with
// TEST.SOFT_NMS / TEST.BBOX_VOTE of test.py:766-779, one Soft-NMS block and one voting wave set per class), one limit+emit kernel; the keypoint net then runs on the device-resident `keypoint_rois`.
//
// Arithmetic is fp32 in NumPy's operation order (this file is compiled with -ffp-contract=off): `rois / im_scale` is a float32
// division by float32(scale) (value-based casting of the reference's NumPy 1.14, test.py:216), `boxes * im_scale` for the
// keypoint rois is formed in float64 and rounded once (test.py:98,121); exp is evaluated in double and rounded once
// (NumPy's float32 exp is within 1 ulp of that).
#include "dat_common.h"
#include "nms_internal.h"

namespace {

constexpr int DET_MAX_T = 16;
constexpr int SEL_THREADS = 1024;

constexpr int MAX_IMAGES = DAT_MAX_IMAGES;

// One block per image (blockIdx.x): image i owns rows [i * roi_cap, (i + 1) * roi_cap) of rois / prob / pred, the count n_rois[i]
// and the scratch at + i * img_ws bytes.
struct DetParams {
    const float* rois;      // [n_images * roi_cap, 4T+1]
    const int* n_rois;      // device counts [n_images]
    const float* prob;      // [R, prob_ld]
    const float* pred;      // [R, pred_ld]
    int prob_ld, pred_ld, roi_cap, T, K, cls_agnostic;
    float wx, wy, ww, wh, xform_clip, score_thresh;
    size_t img_ws;
    double im_scale[MAX_IMAGES];
    float im_h[MAX_IMAGES], im_w[MAX_IMAGES];       // the UNSCALED image (clip bounds, test.py:229)
};

// one tube of class j for roi r: boxes.py:141-183 per frame, then clip (:243-253)
// (TM: compile-time bound of the tube length -- 1 keeps the box in registers, the general instantiation's array lives in scratch;
//  see proposals.hip decode_tube)
template <int TM>
__device__ void decode_tube(const DetParams& p, int img, int r, int j, float* out) {
    const int PT = TM == 1 ? 1 : p.T;
    const int cols = 4 * PT + 1;
    const float im_w = dat_pick(p.im_w, img), im_h = dat_pick(p.im_h, img);
    const int dcls = p.cls_agnostic ? (p.K - 1) : j;       // CLS_AGNOSTIC_BBOX_REG: the last 4T columns (test.py:224-225)
#pragma unroll
    for (int t = 0; t < (TM == 1 ? 1 : PT); ++t) {
        const float* rb = p.rois + (size_t)r * cols + 1 + 4 * t;
        // `rois[:, 1:] / im_scales[0]`: float32 / float32(scale) under the reference environment's NumPy 1.14 casting
        const float sc = (float)dat_pick(p.im_scale, img);
        const float x1 = rb[0] / sc, y1 = rb[1] / sc, x2 = rb[2] / sc, y2 = rb[3] / sc;
        const float* d = p.pred + (size_t)r * p.pred_ld + ((size_t)dcls * PT + t) * 4;
        const float w = x2 - x1 + 1.0f, h = y2 - y1 + 1.0f;
        const float cx = x1 + 0.5f * w, cy = y1 + 0.5f * h;
        const float dx = d[0] / p.wx, dy = d[1] / p.wy;
        const float dw = fminf(d[2] / p.ww, p.xform_clip), dh = fminf(d[3] / p.wh, p.xform_clip);
        const float pcx = dx * w + cx, pcy = dy * h + cy;
        const float pw = (float)exp((double)dw) * w, ph = (float)exp((double)dh) * h;
        float ox1 = pcx - 0.5f * pw, oy1 = pcy - 0.5f * ph, ox2 = pcx + 0.5f * pw, oy2 = pcy + 0.5f * ph;
        ox1 = fmaxf(fminf(ox1, im_w - 1.f), 0.f);
        oy1 = fmaxf(fminf(oy1, im_h - 1.f), 0.f);
        ox2 = fmaxf(fminf(ox2, im_w - 1.f), 0.f);
        oy2 = fmaxf(fminf(oy2, im_h - 1.f), 0.f);
        out[4 * t + 0] = ox1; out[4 * t + 1] = oy1; out[4 * t + 2] = ox2; out[4 * t + 3] = oy2;
    }
}

// block-wide exclusive scan of one value per thread (SEL_THREADS threads); returns the exclusive prefix, *total = sum
__device__ unsigned block_scan(unsigned v, unsigned* scan, unsigned* total) {
    const int tid = threadIdx.x;
    scan[tid] = v;
    __syncthreads();
    for (int off = 1; off < SEL_THREADS; off <<= 1) {
        const unsigned a = (tid >= off) ? scan[tid - off] : 0u;
        __syncthreads();
        scan[tid] += a;
        __syncthreads();
    }
    const unsigned incl = scan[tid];
    *total = scan[SEL_THREADS - 1];
    __syncthreads();
    return incl - v;
}

// ---- per class: inds = where(scores[:, j] > thresh); dets_j = [decoded boxes[inds], scores[inds]]  (test.py:759-762), in roi order
template <int TM>
__global__ __launch_bounds__(SEL_THREADS) void det_select_kernel(const DetParams p, int j, float* dets, int* n_sel) {
    __shared__ unsigned scan[SEL_THREADS];
    const int img = blockIdx.x;
    const int n = min(p.n_rois[img], p.roi_cap);
    const int PT = TM == 1 ? 1 : p.T;
    const int cols = 4 * PT + 1;
    const int per = (n + SEL_THREADS - 1) / SEL_THREADS;
    const int r0 = img * p.roi_cap;              // this image's first row
    const int lo = r0 + threadIdx.x * per, hi = min(r0 + n, lo + per);
    dets = (float*)((char*)dets + (size_t)img * p.img_ws);
    n_sel = (int*)((char*)n_sel + (size_t)img * p.img_ws);
    unsigned local = 0;
    for (int r = lo; r < hi; ++r) local += p.prob[(size_t)r * p.prob_ld + j] > p.score_thresh ? 1u : 0u;
    unsigned total;
    unsigned pos = block_scan(local, scan, &total);
    float tube[4 * TM];
    for (int r = lo; r < hi; ++r) {
        const float sc = p.prob[(size_t)r * p.prob_ld + j];
        if (sc > p.score_thresh) {
            decode_tube<TM>(p, img, r, j, tube);
            float* o = dets + (size_t)pos * cols;
#pragma unroll
            for (int c = 0; c < (TM == 1 ? 4 : 4 * PT); ++c) o[c] = tube[c];
            o[4 * PT] = sc;
            ++pos;
        }
    }
    if (threadIdx.x == 0) *n_sel = (int)total;
}

struct EmitParams {
    const float* dets;     // [K-1][cap][4T+1] selected dets per foreground class
    const int* keep;       // [K-1][cap] kept rows (NMS output order)
    const int* n_keep;     // [K-1]
    int K, T, cap, D, out_cap;
    size_t img_ws;         // image i (blockIdx.x): dets / keep / n_keep at + i * img_ws bytes, outputs at slot i
    double im_scale[MAX_IMAGES];
    float* dets_out;       // [n_images][out_cap][4T+2]: box, score, class
    float* kp_rois;        // [n_images][out_cap][4T+1]: batch index (image i), box * im_scale
    int* n_out;            // [n_images][2]: rows written (<= out_cap), rows the limit rule keeps
};

// ---- DETECTIONS_PER_IM (test.py:790-800): thresh = the D-th best kept score over all classes, keep score >= thresh; then the
// class-major stack (test.py:802) and its keypoint rois.  One block; the D-th best score comes from an exact radix select on the
// float bits (scores are probabilities > 0: the bit pattern is monotonic).
__global__ __launch_bounds__(SEL_THREADS) void det_limit_emit_kernel(const EmitParams pin) {
    EmitParams p = pin;
    const int img = blockIdx.x;
    {
        const size_t o = (size_t)img * p.img_ws;
        p.dets = (const float*)((const char*)p.dets + o);
        p.keep = (const int*)((const char*)p.keep + o);
        p.n_keep = (const int*)((const char*)p.n_keep + o);
        p.dets_out += (size_t)img * p.out_cap * (4 * p.T + 2);
        p.kp_rois += (size_t)img * p.out_cap * (4 * p.T + 1);
        p.n_out += 2 * img;
    }
    const double im_scale = dat_pick(pin.im_scale, img);
    __shared__ unsigned scan[SEL_THREADS];
    __shared__ unsigned hist[256];
    __shared__ unsigned s_prefix, s_need;
    const int tid = threadIdx.x;
    const int cols = 4 * p.T + 1;
    const int nc = p.K - 1;
    int total = 0;
    for (int c = 0; c < nc; ++c) total += p.n_keep[c];
    unsigned thr_bits = 0u;      // keep everything
    if (p.D > 0 && total > p.D) {
        if (tid == 0) { s_prefix = 0u; s_need = (unsigned)p.D; }
        __syncthreads();
        for (int d = 3; d >= 0; --d) {
            if (tid < 256) hist[tid] = 0u;
            __syncthreads();
            const unsigned prefix = s_prefix;
            const int shift = 8 * d;
            const unsigned himask = d == 3 ? 0u : (0xFFFFFFFFu << (shift + 8));
            for (int c = 0; c < nc; ++c) {
                const int m = p.n_keep[c];
                for (int i = tid; i < m; i += SEL_THREADS) {
                    const int row = p.keep[(size_t)c * p.cap + i];
                    const unsigned v = __float_as_uint(p.dets[((size_t)c * p.cap + row) * cols + 4 * p.T]);
                    if ((v & himask) == (prefix & himask)) atomicAdd(&hist[(v >> shift) & 255u], 1u);
                }
            }
            __syncthreads();
            if (tid == 0) {
                unsigned rem = s_need, cum = 0;
                int dig = 255;
                for (; dig >= 0; --dig) {
                    if (cum + hist[dig] >= rem) break;
                    cum += hist[dig];
                }
                s_need = rem - cum;
                s_prefix = prefix | ((unsigned)dig << shift);
            }
            __syncthreads();
        }
        thr_bits = s_prefix;     // the D-th largest score
    }
    // ordered emit: classes in order, kept rows in NMS output order
    unsigned base = 0;
    for (int c = 0; c < nc; ++c) {
        const int m = p.n_keep[c];
        const int per = (m + SEL_THREADS - 1) / SEL_THREADS;
        const int lo = tid * per, hi = min(m, lo + per);
        unsigned local = 0;
        for (int i = lo; i < hi; ++i) {
            const int row = p.keep[(size_t)c * p.cap + i];
            local += __float_as_uint(p.dets[((size_t)c * p.cap + row) * cols + 4 * p.T]) >= thr_bits ? 1u : 0u;
        }
        unsigned tot;
        unsigned pos = base + block_scan(local, scan, &tot);
        for (int i = lo; i < hi; ++i) {
            const int row = p.keep[(size_t)c * p.cap + i];
            const float* src = p.dets + ((size_t)c * p.cap + row) * cols;
            if (__float_as_uint(src[4 * p.T]) >= thr_bits) {
                if ((int)pos < p.out_cap) {
                    float* o = p.dets_out + (size_t)pos * (cols + 1);
                    float* k = p.kp_rois + (size_t)pos * cols;
                    k[0] = (float)img;   // single scale: pyramid level 0 (test.py:106-123) of image `img` of the batch
                    for (int q = 0; q < 4 * p.T; ++q) {
                        o[q] = src[q];
                        k[1 + q] = (float)((double)src[q] * im_scale);
                    }
                    o[4 * p.T] = src[4 * p.T];
                    o[4 * p.T + 1] = (float)(c + 1);
                }
                ++pos;
            }
        }
        base += tot;
    }
    // rows past the kept ones: zero rois (the keypoint net runs on all out_cap rows)
    for (int i = (int)base * cols + tid; i < p.out_cap * cols; i += SEL_THREADS) p.kp_rois[i] = 0.f;
    for (int i = (int)base * (cols + 1) + tid; i < p.out_cap * (cols + 1); i += SEL_THREADS) p.dets_out[i] = 0.f;
    if (tid == 0) {
        p.n_out[0] = min((int)base, p.out_cap);
        p.n_out[1] = (int)base;
    }
}

inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// ---- Soft-NMS on the device, for boxes and tubes: rows of 4T coordinates + score, T = 1 being lib/utils/cython_nms.pyx:98-203
// (include/dat_hip.h, DESIGN.md sections 3.3 and 3.13; the host twin is dat_soft_nms_tubes_host below) ------------------------------
// One block per (image, class).  The class's rows and their original indices stay in LDS (structure of arrays) for the whole greedy
// loop.  Iteration i of the reference:
//   1. arg-max of the scores at positions [i, N) -- strict `<` scan, so the EARLIEST position wins a tie -- swapped into position i;
//   2. positions (i, N) are re-scored against row i, one after the other; a row whose new score is < threshold is overwritten by
//      row N - 1, N shrinks and the slot is visited again.
// Each re-score depends on row i and the position's own row only, so step 2 is: re-score all positions in parallel, then put the
// rows where the serial swap-with-last walk leaves them (positions decide later ties): with N' = N - #removed, survivors below N'
// stay, and the holes below N', in ascending order, receive the surviving rows at positions >= N' in DESCENDING order (the walk
// pulls row N - 1, N - 2, ... into the current hole, dropping the pulled rows that die there).  tests/test_soft_nms_cpu.py pins
// this restatement to dat_soft_nms_host on tie-heavy inputs.
// Every loop is bounded by the row count read once at entry (<= the rows in LDS, checked on the host): a wrong arrangement is a
// mismatch, never a hang.
constexpr int SOFT_THREADS = 256;
constexpr int SOFT_WAVES = SOFT_THREADS / 64;
constexpr int SOFT_NMS_CAP = DAT_SOFT_NMS_MAX_BOXES;

struct SoftParams {
    const float* dets;      // rows [n, 4T+1]; block (img, c) reads dets + img * img_stride bytes + c * cls_stride floats
    const int* n_dev;       // device row counts (n_dev + img * img_stride bytes + c), or nullptr: n_host rows
    float* out;             // re-scored rows in selection order, same addressing as dets
    int* inds;              // original row of every output row (nullable), [cap] per class
    int* ident;             // nullable: ident[k] = k for the output rows (the `keep` list det_limit_emit_kernel walks)
    int* n_out;             // rows left, addressed like n_dev
    size_t img_stride;
    int cls_stride, cap, n_host, method;
    float sigma, Nt, threshold;
    int T;
    int lds_rows;           // rows the launch's dynamic LDS holds (a multiple of 64, >= every row count the block may meet)
};

struct SoftBest { float s; int pos; };
__device__ inline SoftBest soft_better(SoftBest a, SoftBest b) {       // larger score, then the earlier position
    return (b.s > a.s || (b.s == a.s && b.pos < a.pos)) ? b : a;
}

// The overlap of the current maximum row a and a row b: per frame the IoU of cython_nms.pyx:146-160 (`+ 1` is a DOUBLE constant in
// the C that Cython emits: see dat_soft_nms_tubes_host), the T values added in float32 in frame order from 0, divided by (float)T.
// At T = 1 this is the reference's `ov` bit for bit ((0 + x) / 1 == x).  A and B read coordinate c of the two rows.
template <typename A, typename B>
__device__ __forceinline__ float tube_overlap(int T, A a, B b) {
    float sum = 0.f;
    for (int t = 0; t < T; ++t) {
        const float tx1 = a(4 * t + 0), ty1 = a(4 * t + 1), tx2 = a(4 * t + 2), ty2 = a(4 * t + 3);
        const float x1 = b(4 * t + 0), y1 = b(4 * t + 1), x2 = b(4 * t + 2), y2 = b(4 * t + 3);
        const double tarea = ((double)(tx2 - tx1) + 1.0) * ((double)(ty2 - ty1) + 1.0);
        const float area = (float)(((double)(x2 - x1) + 1.0) * ((double)(y2 - y1) + 1.0));
        const float iw = (float)((double)(fminf(tx2, x2) - fmaxf(tx1, x1)) + 1.0);
        const float ih = (float)((double)(fminf(ty2, y2) - fmaxf(ty1, y1)) + 1.0);
        float iou = 0.f;
        if (iw > 0 && ih > 0) {
            const float ua = (float)((tarea + (double)area) - (double)(iw * ih));
            iou = iw * ih / ua;
        }
        sum = sum + iou;
    }
    return sum / (float)T;
}

// Row s of the [words][stride] image to row d != s.  The two rows share no word, which `__restrict__` tells the compiler: it may load
// every word before it stores the first, instead of waiting for each load in turn.
__device__ __forceinline__ void soft_copy_row(float* __restrict__ d, const float* __restrict__ s, int words, int stride) {
    for (int w = 0; w < words; ++w) d[w * stride] = s[w * stride];
}

// Dynamic LDS of soft_nms_kernel for `rows` rows (a multiple of 64): ROWS [4T+2][rows + 1] words (4T coordinates, the score, the
// original index), HOLE [rows] shorts, DEAD [rows] bytes = 16T + 11 bytes a row, and the stage of the swap: row `rows` of ROWS and
// SOFT_WAVES more rows of 4T + 2 words.  The capacity rule counts the rows alone against SOFT_LDS_BUDGET; the 512 bytes it leaves
// of the 160 KB a gfx950 workgroup gets hold the kernel's static LDS and, at the one T whose rows come that close (T = 5: 768
// bytes left), the stage's 440 bytes.
constexpr int SOFT_LDS_BUDGET = 160 * 1024 - 512;
constexpr int SOFT_LDS_STATIC = 304;        // at least the static LDS the compiler reports for soft_nms_kernel
constexpr int SOFT_LDS_DYNAMIC_MAX = 160 * 1024 - SOFT_LDS_STATIC;
constexpr int soft_tube_capacity(int T) {
    if (T < 1 || T > DET_MAX_T) return 0;
    const int rows = SOFT_LDS_BUDGET / (16 * T + 11) / 64 * 64;
    return rows < SOFT_NMS_CAP ? rows : SOFT_NMS_CAP;
}
constexpr int soft_lds_bytes(int rows, int T) { return rows * (16 * T + 11) + (SOFT_WAVES + 1) * (4 * T + 2) * 4; }
constexpr bool soft_lds_fits() {
    for (int T = 1; T <= DET_MAX_T; ++T)
        if (soft_lds_bytes(soft_tube_capacity(T), T) > SOFT_LDS_DYNAMIC_MAX) return false;
    return true;
}
static_assert(soft_lds_fits(), "the rows at capacity, the stage and the static LDS exceed a workgroup's 160 KB for some T");

// TC: the frame count at compile time -- 1: rows of five columns, where the loops over a row's words unroll and the mean of one
// IoU folds away; 0: p.T (as det_select_kernel's TM).  The body is the same for both.
template <int TC>
__global__ __launch_bounds__(SOFT_THREADS) void soft_nms_kernel(const SoftParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char soft_lds[];
    __shared__ int w_pos[SOFT_WAVES];
    __shared__ unsigned w_scan[SOFT_WAVES];
    const int T = TC ? TC : max(1, min(p.T, DET_MAX_T)), C4 = 4 * T, cols = C4 + 1, RW = C4 + 2;
    const int L = p.lds_rows, S = L + 1;
    // word w of row r is ROWS[w * S + r], so lane q reads consecutive words of every column.  Row L is no position of the loop: it
    // holds row i as it is before the swap.  The index travels as the bits of a float: it is only ever loaded and stored
    float* ROWS = (float*)soft_lds;
    float* SC = ROWS + (size_t)C4 * S;
    float* IDX = SC + S;
    unsigned short* HOLE = (unsigned short*)(IDX + S);
    unsigned char* DEAD = (unsigned char*)(HOLE + L);
    float* STAGE = (float*)(DEAD + L);                      // [SOFT_WAVES][RW]: every wave's arg-max row
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the block's last RW threads move the words of row i, one each (the re-score loop's odd trip goes to the first threads)
    const int col = tid - (SOFT_THREADS - RW);
    const int img = blockIdx.x, c = blockIdx.y;
    const size_t ioff = (size_t)img * p.img_stride;
    const float* src = (const float*)((const char*)p.dets + ioff) + (size_t)c * p.cls_stride;
    float* dst = (float*)((char*)p.out + ioff) + (size_t)c * p.cls_stride;
    int n = p.n_dev ? ((const int*)((const char*)p.n_dev + ioff))[c] : p.n_host;
    n = max(0, min(n, min(p.cap, min(L, SOFT_NMS_CAP))));
    for (int e = tid; e < n * cols; e += SOFT_THREADS) {
        const int r = e / cols, w = e - r * cols;
        ROWS[w * S + r] = src[e];
    }
    for (int r = tid; r < n; r += SOFT_THREADS) IDX[r] = __int_as_float(r);
    __syncthreads();
    int N = n;
    for (int i = 0; i < n; ++i) {              // (N only shrinks; every thread holds the same N)
        if (i >= N) break;
        const float old_w = col >= 0 ? ROWS[col * S + i] : 0.f;
        SoftBest b = {SC[i], i};
        for (int q = i + 1 + tid; q < N; q += SOFT_THREADS) {
            const float s = SC[q];
            if (b.s < s) { b.s = s; b.pos = q; }       // ascending q per thread: the strict `<` of the reference
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            SoftBest o = {__shfl_xor(b.s, off), __shfl_xor(b.pos, off)};
            b = soft_better(b, o);
        }
        // The swap of rows i and maxpos costs no barrier of its own: every wave stages its arg-max row and the last RW threads stage
        // row i, one word each, before the barrier of the block's arg-max.  Behind it the winning wave's stage IS the current row,
        // the same threads put it at position i and their word of the old row i at maxpos, and the one thread that visits maxpos
        // reads the old row i from its staged copy, row L, instead (and stores its score, re-scored, itself)
        for (int w = lane; w < RW; w += 64) STAGE[wave * RW + w] = ROWS[w * S + b.pos];
        if (lane == 0) w_pos[wave] = b.pos;
        if (col >= 0) ROWS[col * S + L] = old_w;
        __syncthreads();
        int bw = 0;
        SoftBest best = {STAGE[C4], w_pos[0]};
#pragma unroll
        for (int w = 1; w < SOFT_WAVES; ++w) {
            const SoftBest o = {STAGE[w * RW + C4], w_pos[w]};
            const SoftBest r = soft_better(best, o);
            if (r.pos != best.pos) bw = w;
            best = r;
        }
        const int maxpos = best.pos;           // i <= maxpos < N
        const float* cur = STAGE + bw * RW;
        if (col >= 0) {
            ROWS[col * S + i] = cur[col];      // nobody reads position i again in this iteration
            if (col != C4) ROWS[col * S + maxpos] = old_w;     // (maxpos == i: the same word again)
        }
        int ndead_local = 0;                   // (a flag: did this thread remove a row)
        for (int q = i + 1 + tid; q < N; q += SOFT_THREADS) {
            const int r = q == maxpos ? L : q;                 // where the row now at q is read from
            float s = SC[r];
            const float ov = tube_overlap(T, [&](int cc) { return cur[cc]; }, [&](int cc) { return ROWS[cc * S + r]; });
            bool dead = false;
            if (ov > 0) {                      // (T = 1: iw > 0 && ih > 0 -- there ua >= both areas > 0 and iw * ih > 0)
                float weight;
                if (p.method == 1) weight = ov > p.Nt ? (float)(1.0 - (double)ov) : 1.f;
                else if (p.method == 2) weight = (float)exp((double)(-(ov * ov) / p.sigma));
                else weight = ov > p.Nt ? 0.f : 1.f;
                s = weight * s;
                dead = s < p.threshold;
            }
            SC[q] = s;
            DEAD[q] = dead ? 1 : 0;
            ndead_local |= dead ? 1 : 0;
        }
        // (the barrier also orders this iteration's LDS accesses, the stage's included, before the next iteration's)
        if (!__syncthreads_or(ndead_local)) continue;
        // ---- compaction: holes below N' (ascending) <- survivors at >= N' (descending).  One block scan of the removed flags gives
        // every removed row its ascending rank r (the holes below N' are the ranks 0 .. #holes - 1) and every survivor at q >= N'
        // its descending rank among the tail's survivors, (N - 1 - q) - #removed above q
        const int span = N - (i + 1);
        const int per = (span + SOFT_THREADS - 1) / SOFT_THREADS;
        const int lo = min(N, i + 1 + tid * per), hi = min(N, lo + per);
        unsigned cnt = 0;
        for (int q = lo; q < hi; ++q) cnt += DEAD[q];
        unsigned incl = cnt;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned u = __shfl_up(incl, off);
            if (lane >= off) incl += u;
        }
        if (lane == 63) w_scan[wave] = incl;
        __syncthreads();
        unsigned before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < SOFT_WAVES; ++w) {
            if (w < wave) before += w_scan[w];
            total += w_scan[w];
        }
        const int ndead = (int)total;
        const int N2 = N - ndead;
        int rank = (int)(before + incl - cnt);             // removed rows before position lo
        for (int q = lo; q < hi; ++q) {
            if (DEAD[q]) {
                if (q < N2) HOLE[rank] = (unsigned short)q;
                ++rank;
            }
        }
        __syncthreads();
        rank = (int)(before + incl - cnt);
        for (int q = lo; q < hi; ++q) {
            if (DEAD[q]) { ++rank; continue; }
            if (q >= N2) {
                // the highest survivor fills the lowest hole; the slot index is in [0, #holes) for every consistent arrangement and
                // is clamped to the rows in LDS for any other
                const int slot = min(max((N - 1 - q) - (ndead - rank), 0), L - 1);
                const int h = min((int)HOLE[slot], L - 1);
                soft_copy_row(ROWS + h, ROWS + q, RW, S);
            }
        }
        N = N2;
        __syncthreads();
    }
    for (int e = tid; e < N * cols; e += SOFT_THREADS) {
        const int r = e / cols, w = e - r * cols;
        dst[e] = ROWS[w * S + r];
    }
    for (int r = tid; r < N; r += SOFT_THREADS) {
        if (p.inds) ((int*)((char*)p.inds + ioff))[(size_t)c * p.cap + r] = __float_as_int(IDX[r]);
        if (p.ident) ((int*)((char*)p.ident + ioff))[(size_t)c * p.cap + r] = r;
    }
    if (tid == 0) ((int*)((char*)p.n_out + ioff))[c] = N;
}

// max_rows: the most rows a block of this launch may meet (checked against the capacity by the callers)
int launch_soft_nms(dat_ctx* ctx, hipStream_t st, SoftParams sp, int T, int max_rows, dim3 grid) {
    sp.T = T;
    sp.lds_rows = min(soft_tube_capacity(T), max(64, (max_rows + 63) / 64 * 64));
    const auto kern = T == 1 ? soft_nms_kernel<1> : soft_nms_kernel<0>;
    const int rc = dat_ensure_lds(ctx, (const void*)kern, SOFT_LDS_DYNAMIC_MAX);
    if (rc != DAT_OK) return rc;
    hipLaunchKernelGGL(kern, grid, dim3(SOFT_THREADS), soft_lds_bytes(sp.lds_rows, T), st, sp);
    return DAT_OK;
}

// ---- box voting on the device (lib/utils/boxes.py:294-310; rows of 4T coordinates + score): every kept row's coordinates become
// the score-weighted mean of the class's selected rows (before NMS, original scores) whose overlap with it (tube_overlap; at T = 1
// lib/utils/cython_bbox.pyx:16-57 in the C float order utils/boxes._iou_matrix restates) is >= thresh; the row's score stays.  One
// wave per kept row, whose coordinate l stays in lane l's register for the whole row (the overlap reads it by a lane broadcast),
// so the row may be overwritten in place.  Lane l visits rows l, l + 64, ... and accumulates its sums in double in that order, then a
// butterfly adds the lanes -- a fixed order, so runs repeat bit for bit -- and the mean is rounded to float once.  The 4T + 1 sums
// are formed VOTE_CHUNK frames at a time (16 coordinate sums + the weight sum in registers); a row of more than VOTE_CHUNK frames
// walks the voters once per chunk and finds the same voter set each time (the overlap depends on registers and on `all` only).
constexpr int VOTE_THREADS = 256;
constexpr int VOTE_BLOCKS = 16;
constexpr int VOTE_CHUNK = 4;

struct VoteParams {
    const float* top;       // kept rows [., 4T+1]: row k is top[keep ? keep[k] : k]; addressing as SoftParams
    const int* keep;        // nullable, [cap] per class
    const int* n_top;       // device counts (nullable: n_top_host)
    const float* all;       // the class's selected rows [., 4T+1]
    const int* n_all;       // device counts (nullable: n_all_host)
    float* out;             // [., 4T+1] voted rows, row k (may alias top when keep == nullptr)
    int* ident;             // nullable: ident[k] = k
    size_t img_stride;
    int cls_stride, cap, n_top_host, n_all_host;
    float thresh;
    int T;
};

template <int TC>       // (TC: as soft_nms_kernel's)
__global__ __launch_bounds__(VOTE_THREADS) void box_vote_kernel(const VoteParams p) {
    const int T = TC ? TC : max(1, min(p.T, DET_MAX_T)), C4 = 4 * T, cols = C4 + 1;
    const int lane = threadIdx.x & 63;
    const int img = blockIdx.x, c = blockIdx.y;
    const size_t ioff = (size_t)img * p.img_stride;
    const size_t coff = (size_t)c * p.cls_stride;
    const float* top = (const float*)((const char*)p.top + ioff) + coff;
    const float* all = (const float*)((const char*)p.all + ioff) + coff;
    float* out = (float*)((char*)p.out + ioff) + coff;
    const int n_top = p.n_top ? ((const int*)((const char*)p.n_top + ioff))[c] : p.n_top_host;
    const int n_all = p.n_all ? ((const int*)((const char*)p.n_all + ioff))[c] : p.n_all_host;
    const int* keep = p.keep ? (const int*)((const char*)p.keep + ioff) + (size_t)c * p.cap : nullptr;
    int* ident = p.ident ? (int*)((char*)p.ident + ioff) + (size_t)c * p.cap : nullptr;
    const int wpb = VOTE_THREADS / 64;
    for (int k = blockIdx.z * wpb + (threadIdx.x >> 6); k < n_top; k += gridDim.z * wpb) {      // (k is the same in every lane of a wave)
        const float* t = top + (size_t)(keep ? keep[k] : k) * cols;
        const float mine = lane < C4 ? t[lane] : 0.f;          // lane l: coordinate l of the kept row (4T <= 64 lanes)
        const float bs = t[C4];
        for (int f0 = 0; f0 < T; f0 += VOTE_CHUNK) {
            const int c0 = 4 * f0;
            double sw = 0., sc[4 * VOTE_CHUNK];
#pragma unroll
            for (int j = 0; j < 4 * VOTE_CHUNK; ++j) sc[j] = 0.;
            for (int m = lane; m < n_all; m += 64) {
                const float* q = all + (size_t)m * cols;
                const double dw = (double)q[C4];
                const float ov = tube_overlap(T, [&](int cc) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine), cc)); },
                                              [&](int cc) { return q[cc]; });
                if (ov >= p.thresh) {
                    sw += dw;
#pragma unroll
                    for (int j = 0; j < 4 * VOTE_CHUNK; ++j)
                        if (c0 + j < C4) sc[j] += dw * (double)q[c0 + j];
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                sw += __shfl_xor(sw, off);
#pragma unroll
                for (int j = 0; j < 4 * VOTE_CHUNK; ++j) sc[j] += __shfl_xor(sc[j], off);
            }
            // In-place use: `out` may be `top` (Soft-NMS + voting) and `ident` may be `keep` (NMS + voting).  Only this wave touches row k
            // of either, every lane has loaded its word of t[] and keep[k] before the first butterfly, which keeps the wave in step, so
            // lane 0's stores cannot overtake another lane's load; and no later chunk reads t[] again.
            if (lane == 0) {
                float* o = out + (size_t)k * cols;
#pragma unroll
                for (int j = 0; j < 4 * VOTE_CHUNK; ++j)
                    if (c0 + j < C4) o[c0 + j] = (float)(sc[j] / sw);
            }
        }
        if (lane == 0) {
            out[(size_t)k * cols + C4] = bs;
            if (ident) ident[k] = k;
        }
    }
}

void launch_box_vote(hipStream_t st, const VoteParams& vp, dim3 grid) {
    hipLaunchKernelGGL(vp.T == 1 ? box_vote_kernel<1> : box_vote_kernel<0>, grid, dim3(VOTE_THREADS), 0, st, vp);
}

}  // namespace

extern "C" {

size_t dat_box_results_workspace_bytes(int roi_cap, int num_classes, int T) {
    const int nc = num_classes > 1 ? num_classes - 1 : 1;
    return align_up((size_t)nc * roi_cap * (4 * T + 1) * 4) + align_up((size_t)nc * roi_cap * 4) + 2 * align_up((size_t)nc * 4) +
           dat_nms_ws_bytes(roi_cap, T);
}

// + the re-scored / voted rows [K-1][roi_cap][5] that Soft-NMS and box voting hand to det_limit_emit_kernel
size_t dat_box_results_ex_workspace_bytes(int roi_cap, int num_classes, int T, const dat_det_opts* o) {
    const size_t base = dat_box_results_workspace_bytes(roi_cap, num_classes, T);
    if (!o || (!o->soft_nms_enabled && !o->bbox_vote_enabled)) return base;
    const int nc = num_classes > 1 ? num_classes - 1 : 1;
    return base + align_up((size_t)nc * roi_cap * (4 * T + 1) * 4);
}

// o == nullptr: hard NMS, no voting (dat_box_results_batch); otherwise at least one of the two switches is on
static int box_results_impl(dat_ctx* ctx, dat_stream s, const float* rois, const int* n_rois, int roi_cap, const float* cls_prob,
                            int prob_ld, const float* bbox_pred, int pred_ld, const dat_det_desc* d, const dat_det_opts* o, int n_images,
                            void* workspace, int out_cap, float* dets_out, float* keypoint_rois, int* n_out) {
    DAT_ENFORCE(ctx, rois && n_rois && cls_prob && bbox_pred && d && workspace && dets_out && keypoint_rois && n_out,
                "box_results: null argument");
    DAT_ENFORCE(ctx, n_images >= 1 && n_images <= MAX_IMAGES, "box_results: %d images per launch (1..%d)", n_images, MAX_IMAGES);
    DAT_ENFORCE(ctx, d->num_classes >= 2 && d->T >= 1 && d->T <= DET_MAX_T, "box_results: %d classes / T %d unsupported", d->num_classes, d->T);
    DAT_ENFORCE(ctx, roi_cap > 0 && roi_cap <= 16384 && out_cap > 0, "box_results: roi capacity %d / output capacity %d out of range", roi_cap, out_cap);
    DAT_ENFORCE(ctx, prob_ld >= d->num_classes && pred_ld >= (d->cls_agnostic_bbox_reg ? 4 * d->T : d->num_classes * 4 * d->T),
                "box_results: row strides %d / %d too small for %d classes x T %d", prob_ld, pred_ld, d->num_classes, d->T);
    hipStream_t st = (hipStream_t)s;
    const int nc = d->num_classes - 1, T = d->T, cols = 4 * T + 1;
    const bool soft = o && o->soft_nms_enabled, vote = o && o->bbox_vote_enabled;
    if (soft || vote) {
        DAT_ENFORCE(ctx, T == 1 || o->tubes_enabled, "box_results: Soft-NMS / box voting are defined for boxes, not for tubes of %d frames", T);
        DAT_ENFORCE(ctx, !soft || (o->soft_nms_method >= 0 && o->soft_nms_method <= 2), "box_results: Soft-NMS method %d (0 hard, 1 linear, 2 gaussian)",
                    soft ? o->soft_nms_method : 0);
        DAT_ENFORCE(ctx, !soft || roi_cap <= soft_tube_capacity(T), "box_results: Soft-NMS holds a class's rows in LDS: roi capacity %d > %d", roi_cap,
                    soft_tube_capacity(T));
    }
    const size_t img_ws = dat_box_results_ex_workspace_bytes(roi_cap, d->num_classes, T, o);
    char* ws = (char*)workspace;
    size_t off = 0;
    float* dets = (float*)(ws + off); off += align_up((size_t)nc * roi_cap * cols * 4);
    int* keep = (int*)(ws + off); off += align_up((size_t)nc * roi_cap * 4);
    int* n_sel = (int*)(ws + off); off += align_up((size_t)nc * 4);
    int* n_keep = (int*)(ws + off); off += align_up((size_t)nc * 4);
    char* nms_ws = ws + off; off += dat_nms_ws_bytes(roi_cap, T);
    float* rows2 = (float*)(ws + off);     // (Soft-NMS / voting only: the workspace ends at nms_ws otherwise)
    DetParams p;
    memset(&p, 0, sizeof(p));
    p.rois = rois; p.n_rois = n_rois; p.prob = cls_prob; p.pred = bbox_pred;
    p.prob_ld = prob_ld; p.pred_ld = pred_ld; p.roi_cap = roi_cap; p.T = T; p.K = d->num_classes;
    p.cls_agnostic = d->cls_agnostic_bbox_reg;
    p.wx = d->reg_weights[0]; p.wy = d->reg_weights[1]; p.ww = d->reg_weights[2]; p.wh = d->reg_weights[3];
    p.xform_clip = d->xform_clip; p.score_thresh = d->score_thresh;
    p.img_ws = img_ws;
    EmitParams e;
    memset(&e, 0, sizeof(e));
    for (int i = 0; i < n_images; ++i) {
        DAT_ENFORCE(ctx, d[i].im_scale > 0.f && d[i].nms_thresh > 0.f, "box_results: im_scale and TEST.NMS must be > 0");
        p.im_scale[i] = e.im_scale[i] = (double)d[i].im_scale_f64;
        p.im_h[i] = (float)d[i].im_h; p.im_w[i] = (float)d[i].im_w;
    }
    const unsigned ni = (unsigned)n_images;
    for (int c = 0; c < nc; ++c) {
        float* dets_c = dets + (size_t)c * roi_cap * cols;
        if (p.T == 1) hipLaunchKernelGGL(det_select_kernel<1>, dim3(ni), dim3(SEL_THREADS), 0, st, p, c + 1, dets_c, n_sel + c);
        else hipLaunchKernelGGL(det_select_kernel<DET_MAX_T>, dim3(ni), dim3(SEL_THREADS), 0, st, p, c + 1, dets_c, n_sel + c);
        if (soft) continue;                // (test.py:766-772: Soft-NMS replaces the NMS)
        int rc = dat_nms_impl_batch(ctx, st, nms_ws, img_ws, dets_c, img_ws / 4, 0, n_sel + c, (int)(img_ws / 4), roi_cap, T, d->nms_thresh,
                                    0, 0, keep + (size_t)c * roi_cap, (int)(img_ws / 4), n_keep + c, (int)(img_ws / 4), n_images);
        if (rc != DAT_OK) return rc;
    }
    if (soft) {
        // every (image, class) at once: rows2 = the re-scored rows in selection order, keep = 0, 1, 2, ... over them
        SoftParams sp;
        memset(&sp, 0, sizeof(sp));
        sp.dets = dets; sp.n_dev = n_sel; sp.out = rows2; sp.ident = keep; sp.n_out = n_keep; sp.img_stride = img_ws;
        sp.cls_stride = roi_cap * cols; sp.cap = roi_cap; sp.method = o->soft_nms_method; sp.sigma = o->soft_nms_sigma;
        sp.Nt = d->nms_thresh; sp.threshold = o->soft_nms_score_thresh;
        if (int rc = launch_soft_nms(ctx, st, sp, T, roi_cap, dim3(ni, nc))) return rc;
    }
    if (vote) {
        // (test.py:776-779) the kept rows -- dets[keep] after the NMS, rows2 after Soft-NMS -- voted by the class's selected rows
        VoteParams vp;
        memset(&vp, 0, sizeof(vp));
        vp.top = soft ? rows2 : dets; vp.keep = soft ? nullptr : keep; vp.n_top = n_keep; vp.all = dets; vp.n_all = n_sel;
        vp.out = rows2; vp.ident = soft ? nullptr : keep; vp.img_stride = img_ws; vp.cls_stride = roi_cap * cols; vp.cap = roi_cap;
        vp.thresh = o->bbox_vote_thresh; vp.T = T;
        launch_box_vote(st, vp, dim3(ni, nc, VOTE_BLOCKS));
    }
    e.dets = (soft || vote) ? rows2 : dets; e.keep = keep; e.n_keep = n_keep; e.K = d->num_classes; e.T = T; e.cap = roi_cap; e.D = d->detections_per_im;
    e.out_cap = out_cap; e.img_ws = img_ws; e.dets_out = dets_out; e.kp_rois = keypoint_rois; e.n_out = n_out;
    hipLaunchKernelGGL(det_limit_emit_kernel, dim3(ni), dim3(SEL_THREADS), 0, st, e);
    DAT_CHECK_LAUNCH(ctx, "box_results");
    return DAT_OK;
}

int dat_box_results_batch(dat_ctx* ctx, dat_stream s, const float* rois, const int* n_rois, int roi_cap, const float* cls_prob,
                          int prob_ld, const float* bbox_pred, int pred_ld, const dat_det_desc* d, int n_images, void* workspace,
                          int out_cap, float* dets_out, float* keypoint_rois, int* n_out) {
    return box_results_impl(ctx, s, rois, n_rois, roi_cap, cls_prob, prob_ld, bbox_pred, pred_ld, d, nullptr, n_images, workspace, out_cap,
                            dets_out, keypoint_rois, n_out);
}

int dat_box_results_ex(dat_ctx* ctx, dat_stream s, const float* rois, const int* n_rois, int roi_cap, const float* cls_prob, int prob_ld,
                       const float* bbox_pred, int pred_ld, const dat_det_desc* d, const dat_det_opts* o, int n_images, void* workspace,
                       int out_cap, float* dets_out, float* keypoint_rois, int* n_out) {
    DAT_ENFORCE(ctx, o, "box_results_ex: null options");
    const bool plain = !o->soft_nms_enabled && !o->bbox_vote_enabled;     // both off: dat_box_results_batch itself
    return box_results_impl(ctx, s, rois, n_rois, roi_cap, cls_prob, prob_ld, bbox_pred, pred_ld, d, plain ? nullptr : o, n_images, workspace,
                            out_cap, dets_out, keypoint_rois, n_out);
}

// Soft-NMS of n <= dat_soft_nms_tubes_max_boxes(T) device rows [n, 4T+1]: the device twin of dat_soft_nms_tubes_host below.
// `who`: the entry point the caller used, for the error texts.
static int soft_nms_impl(dat_ctx* ctx, const char* who, dat_stream s, const float* dets, int n, int T, float sigma, float Nt, float threshold,
                         int method, float* dets_out, int* inds_out, int* n_out) {
    DAT_ENFORCE(ctx, dets_out && inds_out && n_out && (dets || n == 0), "%s: null argument", who);
    DAT_ENFORCE(ctx, T >= 1 && T <= DET_MAX_T, "%s: T %d (1..%d)", who, T, DET_MAX_T);
    DAT_ENFORCE(ctx, n >= 0 && n <= soft_tube_capacity(T), "%s: %d rows of %d frames (0..%d: the rows stay in LDS)", who, n, T,
                soft_tube_capacity(T));
    DAT_ENFORCE(ctx, method >= 0 && method <= 2, "%s: method %d (0 hard, 1 linear, 2 gaussian)", who, method);
    SoftParams sp;
    memset(&sp, 0, sizeof(sp));
    sp.dets = dets; sp.n_host = n; sp.out = dets_out; sp.inds = inds_out; sp.n_out = n_out; sp.cap = soft_tube_capacity(T);
    sp.method = method; sp.sigma = sigma; sp.Nt = Nt; sp.threshold = threshold;
    const int rc = launch_soft_nms(ctx, (hipStream_t)s, sp, T, n, dim3(1, 1));
    if (rc != DAT_OK) return rc;
    DAT_CHECK_LAUNCH(ctx, who);
    return DAT_OK;
}

// Voting of n_top device rows [n_top, 4T+1] by n_all device rows [n_all, 4T+1] -> out [n_top, 4T+1] (out may be top_dets).
static int box_voting_impl(dat_ctx* ctx, const char* who, dat_stream s, const float* top_dets, int n_top, const float* all_dets, int n_all,
                           int T, float thresh, float* out) {
    DAT_ENFORCE(ctx, n_top >= 0 && n_all >= 0 && (n_top == 0 || (top_dets && all_dets && out)), "%s: null argument or negative count", who);
    DAT_ENFORCE(ctx, T >= 1 && T <= DET_MAX_T, "%s: T %d (1..%d)", who, T, DET_MAX_T);
    if (n_top == 0) return DAT_OK;
    DAT_ENFORCE(ctx, n_all >= 1, "%s: %d rows to refine and no row to vote with (the weight sum would be zero)", who, n_top);
    VoteParams vp;
    memset(&vp, 0, sizeof(vp));
    vp.top = top_dets; vp.all = all_dets; vp.out = out; vp.n_top_host = n_top; vp.n_all_host = n_all; vp.thresh = thresh; vp.T = T;
    const int blocks = min((n_top + VOTE_THREADS / 64 - 1) / (VOTE_THREADS / 64), 1024);
    launch_box_vote((hipStream_t)s, vp, dim3(1, 1, blocks));
    DAT_CHECK_LAUNCH(ctx, who);
    return DAT_OK;
}

// (include/dat_hip.h) the box entry points are the tube ones at T = 1
int dat_soft_nms(dat_ctx* ctx, dat_stream s, const float* dets, int n, float sigma, float Nt, float threshold, int method, float* dets_out,
                 int* inds_out, int* n_out) {
    return soft_nms_impl(ctx, "soft_nms", s, dets, n, 1, sigma, Nt, threshold, method, dets_out, inds_out, n_out);
}

int dat_soft_nms_tubes(dat_ctx* ctx, dat_stream s, const float* dets, int n, int T, float sigma, float Nt, float threshold, int method,
                       float* dets_out, int* inds_out, int* n_out) {
    return soft_nms_impl(ctx, "soft_nms_tubes", s, dets, n, T, sigma, Nt, threshold, method, dets_out, inds_out, n_out);
}

int dat_box_voting(dat_ctx* ctx, dat_stream s, const float* top_dets, int n_top, const float* all_dets, int n_all, float thresh, float* out) {
    return box_voting_impl(ctx, "box_voting", s, top_dets, n_top, all_dets, n_all, 1, thresh, out);
}

int dat_box_voting_tubes(dat_ctx* ctx, dat_stream s, const float* top_dets, int n_top, const float* all_dets, int n_all, int T, float thresh,
                         float* out) {
    return box_voting_impl(ctx, "box_voting_tubes", s, top_dets, n_top, all_dets, n_all, T, thresh, out);
}

int dat_soft_nms_tubes_max_boxes(int T) { return soft_tube_capacity(T); }

int dat_box_results(dat_ctx* ctx, dat_stream s, const float* rois, const int* n_rois, int roi_cap, const float* cls_prob, int prob_ld,
                    const float* bbox_pred, int pred_ld, const dat_det_desc* d, void* workspace, int out_cap, float* dets_out,
                    float* keypoint_rois, int* n_out) {
    return dat_box_results_batch(ctx, s, rois, n_rois, roi_cap, cls_prob, prob_ld, bbox_pred, pred_ld, d, 1, workspace, out_cap, dets_out,
                                 keypoint_rois, n_out);
}

// Soft-NMS on the HOST for rows [n, 4T+1] (include/dat_hip.h).  At T = 1 it is lib/utils/cython_nms.pyx:98-203 (caller
// lib/core/nms_wrapper.py:29-46, lib/core/test.py:766-772): the greedy in-place re-scoring loop in C float arithmetic, statement for
// statement what Cython emits for the reference's .pyx (differences in float, `+ 1` and the area products in double, the Gaussian
// weight through a double exp, the discard-by-swap-with-last that makes the result order-dependent).  For tubes the per-pair overlap
// is the float32 mean of the per-frame IoUs in frame order, and a pair is re-scored iff that overlap is > 0 (at T = 1: iff iw > 0 and
// ih > 0, as the .pyx nests it).  Plain host code: the comparison path of soft_nms_kernel above and what core/nms_wrapper.soft_nms
// runs for host arrays (tube rows with HIP.TUBE_SOFT_NMS).
int dat_soft_nms_tubes_host(const float* boxes_in, int n, int T, float sigma, float Nt, float threshold, int method, float* boxes_out,
                            int* inds_out, int* n_out) {
    if (!boxes_in || !boxes_out || !inds_out || !n_out || n < 0 || method < 0 || method > 2 || T < 1 || T > DET_MAX_T) return DAT_ERR_ARG;
    const int C4 = 4 * T, cols = C4 + 1;
    float* b = boxes_out;
    memcpy(b, boxes_in, (size_t)n * cols * sizeof(float));
    for (int i = 0; i < n; ++i) inds_out[i] = i;
    int N = n;
    float tmp[4 * DET_MAX_T + 1];
    for (int i = 0; i < N; ++i) {
        float maxscore = b[(size_t)i * cols + C4];
        int maxpos = i;
        for (int pos = i + 1; pos < N; ++pos)
            if (maxscore < b[(size_t)pos * cols + C4]) { maxscore = b[(size_t)pos * cols + C4]; maxpos = pos; }
        memcpy(tmp, b + (size_t)i * cols, cols * sizeof(float));
        const int ti = inds_out[i];
        memmove(b + (size_t)i * cols, b + (size_t)maxpos * cols, cols * sizeof(float));
        inds_out[i] = inds_out[maxpos];
        memcpy(b + (size_t)maxpos * cols, tmp, cols * sizeof(float));
        inds_out[maxpos] = ti;
        const float* a = b + (size_t)i * cols;
        int pos = i + 1;
        while (pos < N) {
            float* r = b + (size_t)pos * cols;
            float sum = 0.f;
            for (int t = 0; t < T; ++t) {
                const float tx1 = a[4 * t], ty1 = a[4 * t + 1], tx2 = a[4 * t + 2], ty2 = a[4 * t + 3];
                const float x1 = r[4 * t], y1 = r[4 * t + 1], x2 = r[4 * t + 2], y2 = r[4 * t + 3];
                // (`+ 1` is a DOUBLE constant in the C that Cython emits for the .pyx: sums and the area products are formed in double and
                //  rounded once to float where the .pyx assigns a `cdef float`)
                const float area = (float)(((double)(x2 - x1) + 1.0) * ((double)(y2 - y1) + 1.0));
                const float iw = (float)((double)(fminf(tx2, x2) - fmaxf(tx1, x1)) + 1.0);
                float iou = 0.f;
                if (iw > 0) {
                    const float ih = (float)((double)(fminf(ty2, y2) - fmaxf(ty1, y1)) + 1.0);
                    if (ih > 0) {
                        const float ua = (float)((((double)(tx2 - tx1) + 1.0) * ((double)(ty2 - ty1) + 1.0) + (double)area) - (double)(iw * ih));
                        iou = iw * ih / ua;
                    }
                }
                sum = sum + iou;
            }
            const float ov = sum / (float)T;
            if (ov > 0) {
                float weight;
                if (method == 1) weight = ov > Nt ? (float)(1.0 - (double)ov) : 1.f;
                else if (method == 2) weight = (float)exp((double)(-(ov * ov) / sigma));
                else weight = ov > Nt ? 0.f : 1.f;
                r[C4] = weight * r[C4];
                if (r[C4] < threshold) {        // discard: swap with the last row, shrink N, revisit this slot
                    memmove(r, b + (size_t)(N - 1) * cols, cols * sizeof(float));
                    inds_out[pos] = inds_out[N - 1];
                    --N;
                    --pos;
                }
            }
            ++pos;
        }
    }
    *n_out = N;
    return DAT_OK;
}

int dat_soft_nms_host(const float* boxes_in, int n, float sigma, float Nt, float threshold, int method, float* boxes_out,
                      int* inds_out, int* n_out) {
    return dat_soft_nms_tubes_host(boxes_in, n, 1, sigma, Nt, threshold, method, boxes_out, inds_out, n_out);
}

}  // extern "C"
