// Greedy NMS of poses on object keypoint similarity, KRCNN.NMS_OKS (reference lib/utils/keypoints.py:221-263 nms_oks / compute_oks, wired at
// lib/core/test.py:883-890 behind a raise; include/dat_hip.h).
//
// Rows are visited in descending order of their mean logit, ties: the later row first.  A visited row i is kept and removes every row j
// still alive behind it unless OKS(i, j) <= thresh, OKS(i, j) = mean over the T frames of mean_k exp(-(dx^2 + dy^2) / vars[k] /
// (area_i,t + eps) / 2): the squared distance in float32 as NumPy forms it (this file is compiled with -ffp-contract=off), the division
// chain, the exponentials and the sums in double, keypoints in order within frames in order.  oks_term / oks_from_terms below state that
// arithmetic for the host loop (dat_oks_nms_host); the kernel adds the same terms in the same order but forms e with one reciprocal per
// kept row, frame and keypoint (oks_term_inv) and the device exp(): its similarities are within a few ulp of the host loop's.
//
// Kernel: one block of 1024 threads per image.  The rows stay in global memory (cap * 4 * 17T floats: 28 KB at 104 boxes, L2-resident;
// 104 tubes of T = 16 would not fit a workgroup's LDS); LDS holds the sortable score keys, the visiting order, the alive flags, the keep
// list, the current kept row's x / y / reciprocals and the terms of a chunk of pairs.  A round of the greedy loop spreads the (row, frame,
// keypoint) terms of the rows behind the kept one over the block -- a thread per pair would run 17 T double divisions and exponentials
// in a row on two waves -- and one thread per row then adds its terms in order: three barriers per kept row.  The order comes from a
// rank count -- row r goes to position #{j : (key_j, j) > (key_r, r)} -- not from the u64 bitonic sort of proposals.hip: the key is a
// whole double and the index does not fit beside it.  No atomics of any kind: two runs write the same bytes.
#include <math.h>

#include <algorithm>

#include "dat_common.h"

namespace {

constexpr int OKS_K = 17;             // the sigma table below is COCO's 17 person keypoints
constexpr int OKS_MAX_T = 16;
constexpr int OKS_THREADS = 1024;
constexpr int OKS_TERMS = 4096;          // terms of one chunk of pairs in LDS (32 KB): 240 pairs at T = 1, 15 at T = 16

struct OksVars {
    double v[OKS_K];
};

// vars = (sigmas * 2) ** 2 with sigmas = [...] / 10.0, the operations of lib/utils/keypoints.py:248-251 in double
OksVars oks_vars() {
    static const double c[OKS_K] = {.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89};
    OksVars r;
    for (int k = 0; k < OKS_K; ++k) {
        const double sigma = c[k] / 10.0;
        const double two = sigma * 2;
        r.v[k] = two * two;
    }
    return r;
}

// a double as a u64 that orders like it: -0 counts as +0, every NaN as the largest value (np.argsort puts NaN last, [::-1] visits it first)
__host__ __device__ inline unsigned long long oks_key(double s) {
    s = s + 0.0;
    unsigned long long u = 0x7ff8000000000000ull;
    if (s == s) memcpy(&u, &s, sizeof(u));
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// mean of the K * T logits of a row, summed in double in storage order
__host__ __device__ inline double oks_score(const float* logit, int KT) {
    double sum = 0.0;
    for (int c = 0; c < KT; ++c) sum += (double)logit[c];
    return sum / (double)KT;
}

// area of frame t's box of a row with the + 1 convention in float32, then + np.spacing(1) in double (lib/utils/keypoints.py:254, :260)
__host__ __device__ inline double oks_area(const float* box) {
    const float w = box[2] - box[0] + 1.f;
    const float h = box[3] - box[1] + 1.f;
    const float area = w * h;
    return (double)area + 2.220446049250313e-16;
}

// one keypoint's term exp(-e) of row j against the kept row i: var = vars[k], area = oks_area of frame t's box of row i
__host__ __device__ inline double oks_term(float xi, float yi, float xj, float yj, double var, double area) {
    const float dx = xj - xi;
    const float dy = yj - yi;
    const float d2 = dx * dx + dy * dy;
    const double e = (double)d2 / var / area / 2;
    return exp(-e);
}

// the kernel's form of oks_term: inv = 1 / (var * area * 2), one reciprocal per kept row, frame and keypoint in place of two divisions
// per term -- e within a few ulp of the division chain's
__device__ inline double oks_term_inv(float xi, float yi, float xj, float yj, double inv) {
    const float dx = xj - xi;
    const float dy = yj - yi;
    const float d2 = dx * dx + dy * dy;
    return exp(-((double)d2 * inv));
}

// OKS of a pair from its K * T terms (frame-major): keypoints in order within frames in order
__host__ __device__ inline double oks_from_terms(const double* term, int T) {
    double total = 0.0;
    for (int t = 0; t < T; ++t) {
        double sum = 0.0;
        for (int k = 0; k < OKS_K; ++k) sum += term[t * OKS_K + k];
        total += sum / (double)OKS_K;
    }
    return total / (double)T;
}

struct OksParams {
    const float* kps;       // [n_images * cap][4][K * T]
    const float* dets;      // [n_images * cap][det_ld], columns [4T | score | class]
    const int* n_rows;      // n_rows[image * n_rows_stride]
    int* keep;              // [n_images][cap]
    int* n_keep;            // [n_images]
    float* dets_out;        // [n_images * cap][det_ld]
    float* kps_out;         // [n_images * cap][4][K * T]
    int det_ld, n_rows_stride, cap, T;
    double thresh;
    OksVars vars;
};

__global__ __launch_bounds__(OKS_THREADS) void oks_nms_kernel(const OksParams p) {
    __shared__ unsigned long long s_key[DAT_OKS_NMS_MAX_ROWS];
    __shared__ int s_order[DAT_OKS_NMS_MAX_ROWS];
    __shared__ int s_keep[DAT_OKS_NMS_MAX_ROWS];
    __shared__ unsigned char s_alive[DAT_OKS_NMS_MAX_ROWS];
    __shared__ float s_x[OKS_K * OKS_MAX_T], s_y[OKS_K * OKS_MAX_T];
    __shared__ double s_inv[OKS_K * OKS_MAX_T];
    __shared__ double s_vars[OKS_K];
    __shared__ double s_term[OKS_TERMS];

    const int tid = threadIdx.x, img = blockIdx.x;
    const int T = p.T, KT = OKS_K * T, row_f = 4 * KT;
    const int pairs_per_chunk = OKS_TERMS / KT;
    const size_t base = (size_t)img * p.cap;
    const float* kps = p.kps + base * row_f;
    const float* dets = p.dets + base * p.det_ld;
    const int n = min(max(p.n_rows[(size_t)img * p.n_rows_stride], 0), p.cap);      // rows beyond are never read

    if (tid < OKS_K) s_vars[tid] = dat_pick(p.vars.v, tid);
    for (int r = tid; r < n; r += OKS_THREADS) {
        s_key[r] = oks_key(oks_score(kps + (size_t)r * row_f + 2 * KT, KT));
        s_alive[r] = 1;
    }
    __syncthreads();
    // the keys (key, row) are distinct, so the ranks are a permutation of 0 .. n-1
    for (int r = tid; r < n; r += OKS_THREADS) {
        const unsigned long long kr = s_key[r];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const unsigned long long kj = s_key[j];
            rank += (kj > kr || (kj == kr && j > r)) ? 1 : 0;
        }
        s_order[rank] = r;
    }
    __syncthreads();

    // every thread walks the same positions: the flags it reads were written before the barrier that ends the previous round
    int nk = 0;
    for (int pos = 0; pos < n; ++pos) {
        const int i = s_order[pos];
        if (!s_alive[i]) continue;
        // this thread's first term of the round: the coordinates of its row j are requested before the kept row's, so that the two
        // global-memory latencies of a round overlap
        const int np0 = min(pairs_per_chunk, n - pos - 1);
        float xj0 = 0.f, yj0 = 0.f;
        bool live0 = false;
        if (tid < np0 * KT) {
            const int pl = tid / KT, c = tid - pl * KT;
            const int j = s_order[pos + 1 + pl];
            if (s_alive[j]) {
                live0 = true;
                xj0 = kps[(size_t)j * row_f + c];
                yj0 = kps[(size_t)j * row_f + KT + c];
            }
        }
        const float* ki = kps + (size_t)i * row_f;
        for (int c = tid; c < KT; c += OKS_THREADS) {
            const int t = c / OKS_K;
            s_x[c] = ki[c];
            s_y[c] = ki[KT + c];
            s_inv[c] = 1.0 / (s_vars[c - t * OKS_K] * oks_area(dets + (size_t)i * p.det_ld + 4 * t) * 2);
        }
        if (tid == 0) s_keep[nk] = i;
        ++nk;
        __syncthreads();
        // the rows behind `pos`, a chunk of pairs at a time: every thread computes terms (pair, frame, keypoint) into LDS, then one
        // thread per pair adds that pair's terms in order -- the sums of a thread that did everything itself, 17 T times less serial
        for (int q0 = pos + 1; q0 < n; q0 += pairs_per_chunk) {
            const int np = min(pairs_per_chunk, n - q0);
            for (int w = tid; w < np * KT; w += OKS_THREADS) {
                const int pl = w / KT, c = w - pl * KT;
                if (q0 == pos + 1 && w == tid) {
                    if (live0) s_term[w] = oks_term_inv(s_x[c], s_y[c], xj0, yj0, s_inv[c]);
                    continue;
                }
                const int j = s_order[q0 + pl];
                if (!s_alive[j]) continue;
                const float* kj = kps + (size_t)j * row_f;
                s_term[w] = oks_term_inv(s_x[c], s_y[c], kj[c], kj[KT + c], s_inv[c]);
            }
            __syncthreads();
            for (int pl = tid; pl < np; pl += OKS_THREADS) {
                const int j = s_order[q0 + pl];
                if (!s_alive[j]) continue;
                const double oks = oks_from_terms(s_term + pl * KT, T);
                if (!(oks <= p.thresh)) s_alive[j] = 0;        // (`order[where(ovr <= thresh)]` stays: a NaN similarity removes)
            }
            __syncthreads();
        }
    }
    __syncthreads();        // (n == 0: the loop ran no barrier; s_keep is read below)

    if (tid == 0) p.n_keep[img] = nk;
    for (int r = tid; r < p.cap; r += OKS_THREADS) p.keep[base + r] = r < nk ? s_keep[r] : -1;
    float* dets_out = p.dets_out + base * p.det_ld;
    for (int e = tid; e < p.cap * p.det_ld; e += OKS_THREADS) {
        const int r = e / p.det_ld, c = e - r * p.det_ld;
        dets_out[e] = r < nk ? dets[(size_t)s_keep[r] * p.det_ld + c] : 0.f;
    }
    float* kps_out = p.kps_out + base * row_f;
    for (int e = tid; e < p.cap * row_f; e += OKS_THREADS) {
        const int r = e / row_f, c = e - r * row_f;
        kps_out[e] = r < nk ? kps[(size_t)s_keep[r] * row_f + c] : 0.f;
    }
}

}  // namespace

extern "C" {

int dat_oks_nms(dat_ctx* ctx, dat_stream s, const float* kps, const float* dets, int det_ld, const int* n_rows, int n_rows_stride, int cap,
                int n_images, int T, int K, double thresh, int* keep, int* n_keep, float* dets_out, float* kps_out) {
    if (!ctx) return DAT_ERR_ARG;
    DAT_ENFORCE(ctx, T >= 1 && T <= OKS_MAX_T, "dat_oks_nms: T = %d outside 1..%d", T, OKS_MAX_T);
    DAT_ENFORCE(ctx, K == OKS_K, "dat_oks_nms: K = %d, the sigma table has %d keypoints", K, OKS_K);
    DAT_ENFORCE(ctx, cap >= 0 && cap <= DAT_OKS_NMS_MAX_ROWS, "dat_oks_nms: cap = %d outside 0..%d (DAT_OKS_NMS_MAX_ROWS)", cap,
                DAT_OKS_NMS_MAX_ROWS);
    DAT_ENFORCE(ctx, n_images >= 0 && det_ld >= 4 * T && n_rows_stride >= 1, "dat_oks_nms: n_images = %d, det_ld = %d (< 4T?), n_rows_stride = %d",
                n_images, det_ld, n_rows_stride);
    if (n_images == 0) return DAT_OK;
    DAT_ENFORCE(ctx, kps && dets && n_rows && keep && n_keep && dets_out && kps_out, "dat_oks_nms: null pointer");
    DAT_ENFORCE(ctx, dets_out != dets && kps_out != kps, "dat_oks_nms: the gathered rows need buffers of their own");
    OksParams p;
    p.kps = kps, p.dets = dets, p.n_rows = n_rows, p.keep = keep, p.n_keep = n_keep, p.dets_out = dets_out, p.kps_out = kps_out;
    p.det_ld = det_ld, p.n_rows_stride = n_rows_stride, p.cap = cap, p.T = T, p.thresh = thresh, p.vars = oks_vars();
    hipLaunchKernelGGL(oks_nms_kernel, dim3(n_images), dim3(OKS_THREADS), 0, (hipStream_t)s, p);
    DAT_CHECK_LAUNCH(ctx, "oks_nms_kernel");
    return DAT_OK;
}

// The host twin (HOST pointers): the same oks_term / oks_from_terms / oks_score / oks_key in plain C++, the comparison path of the kernel.
int dat_oks_nms_host(const float* kps, const float* boxes, int box_ld, int n, int T, int K, double thresh, int* keep, int* n_keep,
                     double* scores_out, double* oks_out) {
    if (n < 0 || T < 1 || T > OKS_MAX_T || K != OKS_K || box_ld < 4 * T || !n_keep || (n > 0 && (!kps || !boxes || !keep))) return DAT_ERR_ARG;
    const OksVars vars = oks_vars();
    const int KT = OKS_K * T, row_f = 4 * KT;
    std::vector<unsigned long long> key(n);
    std::vector<int> order(n);
    std::vector<char> alive(n, 1);
    for (int r = 0; r < n; ++r) {
        const double sc = oks_score(kps + (size_t)r * row_f + 2 * KT, KT);
        if (scores_out) scores_out[r] = sc;
        key[r] = oks_key(sc);
        order[r] = r;
    }
    std::sort(order.begin(), order.end(), [&](int a, int b) { return key[a] != key[b] ? key[a] > key[b] : a > b; });
    int nk = 0;
    double area[OKS_MAX_T], term[OKS_K * OKS_MAX_T];
    for (int pos = 0; pos < n; ++pos) {
        const int i = order[pos];
        if (!alive[i]) continue;
        keep[nk++] = i;
        const float* ki = kps + (size_t)i * row_f;
        for (int t = 0; t < T; ++t) area[t] = oks_area(boxes + (size_t)i * box_ld + 4 * t);
        for (int q = pos + 1; q < n; ++q) {
            const int j = order[q];
            if (!alive[j]) continue;
            const float* kj = kps + (size_t)j * row_f;
            for (int c = 0; c < KT; ++c) term[c] = oks_term(ki[c], ki[KT + c], kj[c], kj[KT + c], vars.v[c % OKS_K], area[c / OKS_K]);
            const double oks = oks_from_terms(term, T);
            if (oks_out) oks_out[(size_t)i * n + j] = oks;
            if (!(oks <= thresh)) alive[j] = 0;
        }
    }
    *n_keep = nk;
    return DAT_OK;
}

}  // extern "C"
