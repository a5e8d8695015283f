// The trainers' segmentation losses as streaming kernels (include/dlka.h: dlka_seg_loss_*, dlka_seg_eval_counts): nnU-Net's DC_and_CE_loss
// (3D/d_lka_former/training/loss_functions/dice_loss.py:158-194, :304-361) that the 3-D trainer steps per deep-supervision head, the 2-D
// trainer's DiceLoss (2D/utils.py:11-47) and the hard tp / fp / fn counts of run_online_evaluation (Trainer_synapse.py:697-718).
//
//   forward   a lane owns SEG_VEC consecutive voxels of the contiguous axis and reads the K class planes with one wide load each; max, sum of
//             exponentials and p_k stay in registers (K bucketed to 4 / 8 / 16 / 32 as in cl_tiles.hip).  Per (sample, class) it accumulates
//             tp = sum p_k [y = k], sp = sum p_k, sq = sum p_k^2, cnt = sum [y = k], per sample ce = sum (logsumexp - x_y).  Reduction: 8 lanes
//             (DPP), then the workgroup through LDS in lane-group order, one partial row per workgroup in the workspace.
//   finish    adds the partial rows in workgroup order in double precision, writes the statistics, the Dice coefficients, the scalar loss and
//             the backward's per-class scalars.  No atomics, no host read: two runs give the same bits.
//   backward  recomputes the softmax from the logits (nothing of size K * N is saved) and writes the gradient once, in the logits' dtype:
//             g_k = coef0_k + coef1_k p_k + coef2_k [y = k];  grad_j = grad_output * (p_j (g_j - sum_k g_k p_k) + ce_scale (p_j - [y = j])).
//   counts    first-maximum argmax (torch.argmax: NaN wins) against the labels; counted in fp32 per workgroup (exact: a workgroup sees fewer
//             than 2^24 voxels), added as integers.
//
// Memory-bound: the forward reads the logits and the labels once, the backward reads them once and writes the gradient once.  A label that is
// not an integer in [0, K) decodes to -1, which matches no class and indexes nothing.
#include <math.h>

#include "cl_pipeline.h"

DLKA_LAUNCH_COUNTER(g_seg_loss_launches, dlka_seg_loss_launch_count)

namespace dlka {

#define SEG_THREADS 256
#define SEG_GROUPS (SEG_THREADS / 8)   // 8-lane groups per workgroup: rows of the LDS reduction

struct SegArgs {
    int B, K, mode, batch_dice, do_bg;
    long N;
    float smooth, weight_ce, weight_dice;
    float class_weight[DLKA_SEG_LOSS_K_MAX];
};

struct alignas(16) SegI64x2 { int64_t x, y; };

__device__ __forceinline__ int seg_label(float v, int K)
{
    if (!(v >= 0.f && v < (float)K)) return -1;   // NaN fails both
    const int i = (int)v;
    return (float)i == v ? i : -1;
}
__device__ __forceinline__ int seg_label(int64_t v, int K) { return (v >= 0 && v < (int64_t)K) ? (int)v : -1; }

template <int VEC>
__device__ __forceinline__ void seg_load_labels(const float *y, long n, int K, int (&yi)[VEC])
{
    if (VEC == 4) {
        const f32x4 v = act_load4(y, n);
#pragma unroll
        for (int e = 0; e < VEC; ++e) yi[e] = seg_label(v[e], K);
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) yi[e] = seg_label(y[n + e], K);
    }
}
template <int VEC>
__device__ __forceinline__ void seg_load_labels(const int64_t *y, long n, int K, int (&yi)[VEC])
{
    if (VEC == 4) {
        const SegI64x2 lo = *reinterpret_cast<const SegI64x2 *>(y + n), hi = *reinterpret_cast<const SegI64x2 *>(y + n + 2);
        yi[0] = seg_label(lo.x, K); yi[1 % VEC] = seg_label(lo.y, K); yi[2 % VEC] = seg_label(hi.x, K); yi[3 % VEC] = seg_label(hi.y, K);
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) yi[e] = seg_label(y[n + e], K);
    }
}

// the K class planes of VEC consecutive voxels: l[k][e]
template <typename T, int KB, int VEC>
__device__ __forceinline__ void seg_load_logits(const T *xb, long n, long N, int K, float (&l)[KB][VEC])
{
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        if (k < K) {
            if (VEC == 4) {
                const f32x4 v = act_load4(xb, (long)k * N + n);
#pragma unroll
                for (int e = 0; e < VEC; ++e) l[k][e] = v[e];
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e) l[k][e] = act_load1(xb, (long)k * N + n + e);
            }
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) l[k][e] = 0.f;
        }
    }
}

// p = softmax over the first K entries of column e, in place; returns logsumexp
template <int KB, int VEC>
__device__ __forceinline__ float seg_softmax(float (&l)[KB][VEC], int e, int K)
{
    float mx = l[0][e];
#pragma unroll
    for (int k = 1; k < KB; ++k)
        if (k < K) mx = fmaxf(mx, l[k][e]);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < KB; ++k)
        if (k < K) { l[k][e] = expf(l[k][e] - mx); s += l[k][e]; }
    const float inv = 1.f / s;
#pragma unroll
    for (int k = 0; k < KB; ++k)
        if (k < K) l[k][e] *= inv;
    return mx + logf(s);
}

template <typename T, typename L, int KB, int VEC>
__global__ __launch_bounds__(SEG_THREADS) void dlka_seg_loss_fwd_kernel(const SegArgs a, const T *__restrict__ x, const L *__restrict__ y,
                                                                        float *__restrict__ partial)
{
    constexpr int S = 4 * KB + 2;
    __shared__ float red[SEG_GROUPS][S];
    const int tid = threadIdx.x, b = blockIdx.y, g = blockIdx.x, G = gridDim.x;
    const T *xb = x + (long)b * a.K * a.N;
    const L *yb = y + (long)b * a.N;
    float tp[KB] = {}, sp[KB] = {}, sq[KB] = {}, cnt[KB] = {};
    float ce = 0.f, bad = 0.f;
    for (long n = ((long)g * SEG_THREADS + tid) * VEC; n < a.N; n += (long)G * SEG_THREADS * VEC) {   // (N % VEC == 0: a vector never straddles the end)
        float l[KB][VEC];
        int yi[VEC];
        seg_load_logits<T, KB, VEC>(xb, n, a.N, a.K, l);
        seg_load_labels<VEC>(yb, n, a.K, yi);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            float xy = 0.f;
#pragma unroll
            for (int k = 0; k < KB; ++k)
                if (k < a.K && yi[e] == k) xy = l[k][e];
            const float lse = seg_softmax<KB, VEC>(l, e, a.K);
            if (yi[e] >= 0) ce += lse - xy; else bad += 1.f;
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                if (k < a.K) {
                    const float p = l[k][e];
                    const bool hit = yi[e] == k;
                    sp[k] += p;
                    sq[k] += p * p;
                    tp[k] += hit ? p : 0.f;
                    cnt[k] += hit ? 1.f : 0.f;
                }
            }
        }
    }
    // 8 lanes by DPP, then the 32 lane groups through LDS, added in group order
    const bool lead = (tid & 7) == 0;
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        const float v0 = sum8(tp[k]), v1 = sum8(sp[k]), v2 = sum8(sq[k]), v3 = sum8(cnt[k]);
        if (lead) { red[tid >> 3][k] = v0; red[tid >> 3][KB + k] = v1; red[tid >> 3][2 * KB + k] = v2; red[tid >> 3][3 * KB + k] = v3; }
    }
    {
        const float v0 = sum8(ce), v1 = sum8(bad);
        if (lead) { red[tid >> 3][4 * KB] = v0; red[tid >> 3][4 * KB + 1] = v1; }
    }
    __syncthreads();
    const int Sr = 4 * a.K + 2;   // the row as stored: tp[K], sp[K], sq[K], cnt[K], ce, bad
    if (tid < Sr) {
        const int s = tid < 4 * a.K ? (tid / a.K) * KB + tid % a.K : 4 * KB + (tid - 4 * a.K);
        float acc = 0.f;
        for (int r = 0; r < SEG_GROUPS; ++r) acc += red[r][s];
        partial[((long)b * G + g) * Sr + tid] = acc;
    }
}

__global__ __launch_bounds__(SEG_THREADS) void dlka_seg_loss_finish_kernel(const SegArgs a, int G, const float *__restrict__ partial,
                                                                           float *__restrict__ loss, float *__restrict__ dc,
                                                                           float *__restrict__ stats, float *__restrict__ coef)
{
    const int K = a.K, B = a.B, Sr = 4 * K + 2;
    for (int idx = threadIdx.x; idx < B * Sr; idx += SEG_THREADS) {
        const int b = idx / Sr, s = idx % Sr;
        double acc = 0.0;
        for (int g = 0; g < G; ++g) acc += (double)partial[((long)b * G + g) * Sr + s];
        stats[idx] = (float)acc;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    // B * K values: one lane, double precision, fixed order
    double ce = 0.0, bad = 0.0;
    for (int b = 0; b < B; ++b) { ce += (double)stats[b * Sr + 4 * K]; bad += (double)stats[b * Sr + 4 * K + 1]; }
    const double qnan = (double)__uint_as_float(0x7fc00000u);
    double total = 0.0;
    if (a.mode == DLKA_SEG_LOSS_NNUNET) {
        const int rows = a.batch_dice ? 1 : B, k0 = a.do_bg ? 0 : 1;
        const double M = (double)rows * (double)(K - k0), wd = (double)a.weight_dice, sm = (double)a.smooth;
        double dsum = 0.0;
        for (int r = 0; r < rows; ++r)
            for (int k = 0; k < K; ++k) {
                double tp = 0.0, sp = 0.0, cnt = 0.0;
                for (int b = (a.batch_dice ? 0 : r); b < (a.batch_dice ? B : r + 1); ++b) {
                    tp += (double)stats[b * Sr + k]; sp += (double)stats[b * Sr + K + k]; cnt += (double)stats[b * Sr + 3 * K + k];
                }
                const double nom = 2.0 * tp + sm, den = sp + cnt + sm + 1e-8;   // 2 tp + fp + fn = sp + cnt
                const bool use = k >= k0;
                double d = use ? nom / den : 0.0, c0 = use ? wd / M * nom / (den * den) : 0.0, c2 = use ? -wd / M * 2.0 / den : 0.0;
                if (use) dsum += d;
                if (bad > 0.0) { d = qnan; c0 = qnan; c2 = qnan; }
                for (int b = (a.batch_dice ? 0 : r); b < (a.batch_dice ? B : r + 1); ++b) {
                    dc[b * K + k] = (float)d;
                    coef[(b * 3 + 0) * K + k] = (float)c0; coef[(b * 3 + 1) * K + k] = 0.f; coef[(b * 3 + 2) * K + k] = (float)c2;
                }
            }
        const double ce_scale = (double)a.weight_ce / ((double)B * (double)a.N);
        coef[B * 3 * K] = (float)ce_scale;
        total = ce_scale * ce;
        if (a.weight_dice != 0.f) total -= wd * (dsum / M);
        if (bad > 0.0) total = qnan;
    } else {   // DLKA_SEG_LOSS_DICE2D
        for (int k = 0; k < K; ++k) {
            double I = 0.0, Z = 0.0, Y = 0.0;
            for (int b = 0; b < B; ++b) { I += (double)stats[b * Sr + k]; Z += (double)stats[b * Sr + 2 * K + k]; Y += (double)stats[b * Sr + 3 * K + k]; }
            const double nom = 2.0 * I + 1e-5, den = Z + Y + 1e-5, w = (double)a.class_weight[k] / (double)K;
            total += w * (1.0 - nom / den);
            for (int b = 0; b < B; ++b) {
                dc[b * K + k] = (float)(nom / den);
                coef[(b * 3 + 0) * K + k] = 0.f; coef[(b * 3 + 1) * K + k] = (float)(w * 2.0 * nom / (den * den)); coef[(b * 3 + 2) * K + k] = (float)(-w * 2.0 / den);
            }
        }
        coef[B * 3 * K] = 0.f;
    }
    loss[0] = (float)total;
}

template <typename T, typename L, int KB, int VEC>
__global__ __launch_bounds__(SEG_THREADS) void dlka_seg_loss_bwd_kernel(const SegArgs a, const T *__restrict__ x, const L *__restrict__ y,
                                                                        const float *__restrict__ coef, const float *__restrict__ grad_output,
                                                                        T *__restrict__ gx)
{
    const int b = blockIdx.y;
    const long n = ((long)blockIdx.x * SEG_THREADS + threadIdx.x) * VEC;
    if (n >= a.N) return;
    const T *xb = x + (long)b * a.K * a.N;
    T *gb = gx + (long)b * a.K * a.N;
    float c0[KB], c1[KB], c2[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        const bool in = k < a.K;
        c0[k] = in ? coef[(b * 3 + 0) * a.K + k] : 0.f; c1[k] = in ? coef[(b * 3 + 1) * a.K + k] : 0.f; c2[k] = in ? coef[(b * 3 + 2) * a.K + k] : 0.f;
    }
    const float ces = coef[a.B * 3 * a.K], go = grad_output[0];
    float l[KB][VEC];
    int yi[VEC];
    seg_load_logits<T, KB, VEC>(xb, n, a.N, a.K, l);
    seg_load_labels<VEC>(y + (long)b * a.N, n, a.K, yi);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        (void)seg_softmax<KB, VEC>(l, e, a.K);
        float gk[KB];
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            gk[k] = 0.f;
            if (k < a.K) {
                gk[k] = c0[k] + c1[k] * l[k][e] + (yi[e] == k ? c2[k] : 0.f);
                dot += gk[k] * l[k][e];
            }
        }
#pragma unroll
        for (int k = 0; k < KB; ++k)
            if (k < a.K) l[k][e] = go * (l[k][e] * (gk[k] - dot) + ces * (l[k][e] - (yi[e] == k ? 1.f : 0.f)));
    }
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        if (k < a.K) {
            if (VEC == 4) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < VEC; ++e) v[e] = l[k][e];
                act_store4(gb, (long)k * a.N + n, v);
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e) act_store1(gb, (long)k * a.N + n + e, l[k][e]);
            }
        }
    }
}

template <typename T, typename L, int KB, int VEC>
__global__ __launch_bounds__(SEG_THREADS) void dlka_seg_eval_kernel(const SegArgs a, const T *__restrict__ x, const L *__restrict__ y,
                                                                    int *__restrict__ partial)
{
    constexpr int S = 3 * KB;
    __shared__ float red[SEG_GROUPS][S];
    const int tid = threadIdx.x, b = blockIdx.y, g = blockIdx.x, G = gridDim.x;
    const T *xb = x + (long)b * a.K * a.N;
    const L *yb = y + (long)b * a.N;
    float tp[KB] = {}, pr[KB] = {}, cnt[KB] = {};
    for (long n = ((long)g * SEG_THREADS + tid) * VEC; n < a.N; n += (long)G * SEG_THREADS * VEC) {
        float l[KB][VEC];
        int yi[VEC];
        seg_load_logits<T, KB, VEC>(xb, n, a.N, a.K, l);
        seg_load_labels<VEC>(yb, n, a.K, yi);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            float best = l[0][e];
            int idx = 0;
#pragma unroll
            for (int k = 1; k < KB; ++k)
                if (k < a.K && !isnan(best) && (isnan(l[k][e]) || l[k][e] > best)) { best = l[k][e]; idx = k; }
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                const bool p = idx == k, t = yi[e] == k;
                pr[k] += p ? 1.f : 0.f;
                cnt[k] += t ? 1.f : 0.f;
                tp[k] += (p && t) ? 1.f : 0.f;
            }
        }
    }
    const bool lead = (tid & 7) == 0;
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        const float v0 = sum8(tp[k]), v1 = sum8(pr[k]), v2 = sum8(cnt[k]);
        if (lead) { red[tid >> 3][k] = v0; red[tid >> 3][KB + k] = v1; red[tid >> 3][2 * KB + k] = v2; }
    }
    __syncthreads();
    if (tid < 3 * a.K) {
        const int s = (tid / a.K) * KB + tid % a.K;
        float acc = 0.f;
        for (int r = 0; r < SEG_GROUPS; ++r) acc += red[r][s];
        partial[((long)b * G + g) * 3 * a.K + tid] = (int)acc;
    }
}

__global__ __launch_bounds__(64) void dlka_seg_eval_finish_kernel(int B, int K, int G, const int *__restrict__ partial, int64_t *__restrict__ counts)
{
    const int k = 1 + threadIdx.x;
    if (k >= K) return;
    int64_t tp = 0, pr = 0, cnt = 0;
    for (long r = 0; r < (long)B * G; ++r) { tp += partial[r * 3 * K + k]; pr += partial[r * 3 * K + K + k]; cnt += partial[r * 3 * K + 2 * K + k]; }
    counts[k - 1] = tp;
    counts[(K - 1) + k - 1] = pr - tp;
    counts[2 * (K - 1) + k - 1] = cnt - tp;
}

// workgroups per sample of the two reducing launches: enough to fill the device at the trainer's batch sizes, and few enough voxels per
// workgroup for exact fp32 counting
static long seg_groups(const dlka_seg_loss_desc *d, int vec)
{
    long cap = 1024 / d->B;
    cap = cap < 32 ? 32 : (cap > 512 ? 512 : cap);
    const long need = cdivl(d->N, (long)SEG_THREADS * vec), exact = cdivl(d->N, 1L << 23);
    long G = need < cap ? need : cap;
    return G < exact ? exact : G;
}

static int seg_check(const dlka_seg_loss_desc *d)
{
    if (!d) return DLKA_ERR_NULL;
    if (d->B <= 0 || d->K <= 0 || d->N <= 0 || d->B > 65535) return DLKA_ERR_SHAPE;
    if (d->dtype != DLKA_F32 && d->dtype != DLKA_BF16) return DLKA_ERR_DTYPE;
    if (d->label_dtype != DLKA_LABEL_F32 && d->label_dtype != DLKA_LABEL_I64) return DLKA_ERR_DTYPE;
    if (d->K > DLKA_SEG_LOSS_K_MAX || (d->mode != DLKA_SEG_LOSS_NNUNET && d->mode != DLKA_SEG_LOSS_DICE2D)) return DLKA_ERR_UNSUPPORTED;
    if (cdivl(d->N, SEG_THREADS) > 0x7fffffffL || seg_groups(d, 1) > 0x7fffffffL) return DLKA_ERR_UNSUPPORTED;
    return DLKA_OK;
}

// wide loads need vectors that do not straddle a plane or a 16-byte line (8-byte for bf16)
static int seg_vec(const dlka_seg_loss_desc *d, const void *x, const void *y, const void *gx)
{
    if (d->K > 16 || d->N % 4 != 0) return 1;
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)gx) & 15) return 1;
    return 4;
}

static SegArgs seg_args(const dlka_seg_loss_desc *d)
{
    SegArgs a = {};
    a.B = d->B; a.K = d->K; a.N = (long)d->N; a.mode = d->mode; a.batch_dice = d->batch_dice; a.do_bg = d->do_bg;
    a.smooth = d->smooth; a.weight_ce = d->weight_ce; a.weight_dice = d->weight_dice;
    for (int k = 0; k < DLKA_SEG_LOSS_K_MAX; ++k) a.class_weight[k] = d->class_weight[k];
    return a;
}

enum { SEG_FWD, SEG_BWD, SEG_EVAL };
struct SegCall {
    int what;
    const void *x, *y;
    void *out;            // fwd: float partials; bwd: grad_logits; eval: int partials
    const float *coef, *go;
    dim3 grid;
    hipStream_t st;
};

template <typename T, typename L, int KB, int VEC>
static void seg_launch(const SegArgs &a, const SegCall &c)
{
    const T *x = (const T *)c.x;
    const L *y = (const L *)c.y;
    if (c.what == SEG_FWD) { auto k = dlka_seg_loss_fwd_kernel<T, L, KB, VEC>; DLKA_LAUNCH(k, c.grid, dim3(SEG_THREADS), 0, c.st, a, x, y, (float *)c.out); }
    else if (c.what == SEG_BWD) { auto k = dlka_seg_loss_bwd_kernel<T, L, KB, VEC>; DLKA_LAUNCH(k, c.grid, dim3(SEG_THREADS), 0, c.st, a, x, y, c.coef, c.go, (T *)c.out); }
    else { auto k = dlka_seg_eval_kernel<T, L, KB, VEC>; DLKA_LAUNCH(k, c.grid, dim3(SEG_THREADS), 0, c.st, a, x, y, (int *)c.out); }
}

template <typename T, typename L>
static void seg_launch_k(const SegArgs &a, const SegCall &c, int vec)
{
    if (a.K > 16) { seg_launch<T, L, 32, 1>(a, c); return; }   // (4 voxels x 32 classes would not fit the register file)
    if (vec == 4) {
        if (a.K <= 4) seg_launch<T, L, 4, 4>(a, c);
        else if (a.K <= 8) seg_launch<T, L, 8, 4>(a, c);
        else seg_launch<T, L, 16, 4>(a, c);
    } else {
        if (a.K <= 4) seg_launch<T, L, 4, 1>(a, c);
        else if (a.K <= 8) seg_launch<T, L, 8, 1>(a, c);
        else seg_launch<T, L, 16, 1>(a, c);
    }
}

static void seg_dispatch(const dlka_seg_loss_desc *d, const SegArgs &a, const SegCall &c, int vec)
{
    g_seg_loss_launches.add();
    dispatch_storage<ST_F32 | ST_BF16>(d->dtype, [&](auto t) -> int {
        dispatch_bool(d->label_dtype == DLKA_LABEL_I64, [&](auto i64) {
            seg_launch_k<DLKA_T(t), std::conditional_t<DLKA_V(i64), int64_t, float>>(a, c, vec);
        });
        return DLKA_OK;
    });
}

}  // namespace dlka

using namespace dlka;

extern "C" size_t dlka_seg_loss_workspace_bytes(const dlka_seg_loss_desc *d)
{
    if (seg_check(d) != DLKA_OK) return 0;
    const size_t rows = (size_t)d->B * (size_t)seg_groups(d, 1);   // (the scalar layout has the most workgroups)
    const size_t fwd = rows * (size_t)(4 * d->K + 2) * sizeof(float), ev = rows * (size_t)(3 * d->K) * sizeof(int);
    return fwd > ev ? fwd : ev;
}

extern "C" int dlka_seg_loss_forward(const void *logits, const void *labels, const dlka_seg_loss_desc *d, void *workspace, size_t workspace_bytes,
                                     float *loss, float *dc, float *stats, float *coef, void *stream)
{
    const int rc = seg_check(d);
    if (rc != DLKA_OK) return rc;
    if (!logits || !labels || !loss || !dc || !stats || !coef) return DLKA_ERR_NULL;
    if (!workspace || workspace_bytes < dlka_seg_loss_workspace_bytes(d)) return DLKA_ERR_WORKSPACE;
    const SegArgs a = seg_args(d);
    const int vec = seg_vec(d, logits, labels, nullptr);
    const long G = seg_groups(d, vec);
    hipStream_t st = (hipStream_t)stream;
    SegCall c = {SEG_FWD, logits, labels, workspace, nullptr, nullptr, dim3((unsigned)G, (unsigned)d->B), st};
    seg_dispatch(d, a, c, vec);
    DLKA_CHECK_LAUNCH();
    g_seg_loss_launches.add();
    DLKA_LAUNCH(dlka_seg_loss_finish_kernel, dim3(1), dim3(SEG_THREADS), 0, st, a, (int)G, (const float *)workspace, loss, dc, stats, coef);
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}

extern "C" int dlka_seg_loss_backward(const void *logits, const void *labels, const dlka_seg_loss_desc *d, const float *coef, const float *grad_output,
                                      void *grad_logits, void *stream)
{
    const int rc = seg_check(d);
    if (rc != DLKA_OK) return rc;
    if (!logits || !labels || !coef || !grad_output || !grad_logits) return DLKA_ERR_NULL;
    const SegArgs a = seg_args(d);
    const int vec = seg_vec(d, logits, labels, grad_logits);
    SegCall c = {SEG_BWD, logits, labels, grad_logits, coef, grad_output, dim3((unsigned)cdivl(d->N, (long)SEG_THREADS * vec), (unsigned)d->B),
                 (hipStream_t)stream};
    seg_dispatch(d, a, c, vec);
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}

extern "C" int dlka_seg_eval_counts(const void *logits, const void *labels, const dlka_seg_loss_desc *d, void *workspace, size_t workspace_bytes,
                                    int64_t *counts, void *stream)
{
    const int rc = seg_check(d);
    if (rc != DLKA_OK) return rc;
    if (!logits || !labels || !counts) return DLKA_ERR_NULL;
    if (d->K < 2 || d->K - 1 > 64) return DLKA_ERR_SHAPE;   // no foreground class
    if (!workspace || workspace_bytes < dlka_seg_loss_workspace_bytes(d)) return DLKA_ERR_WORKSPACE;
    const SegArgs a = seg_args(d);
    const int vec = seg_vec(d, logits, labels, nullptr);
    const long G = seg_groups(d, vec);
    hipStream_t st = (hipStream_t)stream;
    SegCall c = {SEG_EVAL, logits, labels, workspace, nullptr, nullptr, dim3((unsigned)G, (unsigned)d->B), st};
    seg_dispatch(d, a, c, vec);
    DLKA_CHECK_LAUNCH();
    g_seg_loss_launches.add();
    DLKA_LAUNCH(dlka_seg_eval_finish_kernel, dim3(1), dim3(64), 0, st, (int)d->B, (int)d->K, (int)G, (const int *)workspace, counts);
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}
