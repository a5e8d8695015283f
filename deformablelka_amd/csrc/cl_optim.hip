// The trainers' optimizer step as multi-tensor streaming kernels (include/dlka.h: dlka_optim_*): clip_grad_norm_(12) followed by the SGD /
// momentum / Nesterov step of d_lka_former_trainer_synapse.py:197-205,291-309 (2D/trainer_MaxViT_deform_LKA.py:114, train_pancreas.py:127
// without clipping), with the learning rate read from device memory so that a captured iteration follows the schedule (:451).
//
//   tables    the entries take host arrays of per-tensor pointers and element counts and cut them into launches whose argument struct
//             carries up to DLKA_OPTIM_TENSORS_PER_LAUNCH records BY VALUE: every address is a kernel-node argument (a hipGraph capture holds
//             the gradient addresses of its private pool without a captured copy), and nothing is read from the host arrays after return.
//   partition a workgroup owns one chunk of DLKA_OPTIM_CHUNK elements of one tensor; it finds its tensor by bisection of the table's running
//             chunk counts.  The map depends on the element counts only.  A lane owns OPT_VEC consecutive elements, OPT_ITERS times at a stride
//             of the workgroup: one 16-byte access each where every pointer of the tensor is 16-byte aligned (scalar at the tensor's end),
//             scalar accesses of the same elements otherwise -- the same lane does the same arithmetic on the same element either way.
//   norm      squares summed in float64 in the lane, across the wave by DPP, across the four waves through LDS in wave order, one float64
//             partial per chunk at its global chunk index; a finishing launch adds the partials in a fixed order (lane t takes the indices
//             t, t + 256, ... ascending, then the same wave / LDS reduction) and writes (float)sqrt(sum).  No atomics, no host read.
//   scale     g *= min(1, max_norm / (norm + 1e-6)), the coefficient formed in float32 as torch.nn.utils.clip_grad_norm_ forms it.
//   sgd_step  one visit per element in torch.optim.SGD's order: g_c = g coef; d = g_c + wd p; buf = m buf + d; u = nesterov ? d + m buf : buf;
//             p -= lr u.  The gradient is not written back.
//
// Memory-bound: the norm reads the gradients once; the step reads p, g, buf and writes p, buf.  Contraction is off in this file: the two
// access variants, the emulator and the GPU round every product and every sum separately.
#include <math.h>

#include "cl_pipeline.h"

#pragma clang fp contract(off)

DLKA_LAUNCH_COUNTER(g_optim_launches, dlka_optim_launch_count)

namespace dlka {

#define OPT_THREADS 256
#define OPT_VEC 4
#define OPT_ITERS (DLKA_OPTIM_CHUNK / (OPT_THREADS * OPT_VEC))
static_assert(DLKA_OPTIM_CHUNK % (OPT_THREADS * OPT_VEC) == 0 && OPT_ITERS >= 1, "a chunk is a whole number of workgroup sweeps");

// one launch's tensors: first[i] = chunks of the tensors before i (first[n] = the grid), so zero-element tensors own no workgroup
struct OptimTable {
    int n, chunk_base;   // chunk_base: chunks of the launches before this one (the norm's workspace slot)
    int first[DLKA_OPTIM_TENSORS_PER_LAUNCH + 1];
    int count[DLKA_OPTIM_TENSORS_PER_LAUNCH];
    float *p[DLKA_OPTIM_TENSORS_PER_LAUNCH];
    float *g[DLKA_OPTIM_TENSORS_PER_LAUNCH];
    float *b[DLKA_OPTIM_TENSORS_PER_LAUNCH];
};
struct SgdArgs {
    float momentum, weight_decay, max_norm;
    int nesterov, clip, lr_index;
};
static_assert(sizeof(OptimTable) + sizeof(SgdArgs) + 2 * sizeof(void *) <= 4096, "the kernel-argument budget");

// the tensor of workgroup `blk`: the last i with first[i] <= blk (first[i + 1] > blk, so it owns at least this chunk)
__device__ __forceinline__ int opt_locate(const OptimTable &t, int blk)
{
    int lo = 0, hi = t.n;   // first[lo] <= blk < first[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t.first[mid] <= blk) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool opt_aligned(const void *a, const void *b, const void *c)
{
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

// torch: clip_coef = max_norm / (total_norm + 1e-6); clamp(clip_coef, max=1.0) -- a NaN stays a NaN
__device__ __forceinline__ float opt_clip_coef(float norm, float max_norm)
{
    const float c = max_norm / (norm + 1e-6f);
    return c > 1.f ? 1.f : c;
}

// workgroup sum of one float64 per lane, in wave order; valid in thread 0
__device__ __forceinline__ double opt_block_sum(double acc, double (&red)[OPT_THREADS / 64])
{
    const double w = wave_sum_f64(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int i = 1; i < OPT_THREADS / 64; ++i) s += red[i];
    return s;
}

template <bool VEC> __device__ __forceinline__ double opt_sumsq(const float *__restrict__ g, int len)
{
    float v[OPT_ITERS][OPT_VEC];
#pragma unroll
    for (int j = 0; j < OPT_ITERS; ++j) {
        const int e0 = (j * OPT_THREADS + (int)threadIdx.x) * OPT_VEC;
        if (VEC && e0 + OPT_VEC <= len) {
            const f32x4 q = act_load4(g, e0);
#pragma unroll
            for (int e = 0; e < OPT_VEC; ++e) v[j][e] = q[e];
        } else {
#pragma unroll
            for (int e = 0; e < OPT_VEC; ++e) v[j][e] = e0 + e < len ? g[e0 + e] : 0.f;
        }
    }
    double acc = 0.0;   // (an element past the end adds +0.0: the sum's bits do not depend on the variant)
#pragma unroll
    for (int j = 0; j < OPT_ITERS; ++j)
#pragma unroll
        for (int e = 0; e < OPT_VEC; ++e) acc += (double)v[j][e] * (double)v[j][e];
    return acc;
}

__global__ __launch_bounds__(OPT_THREADS) void dlka_optim_sumsq_kernel(const OptimTable t, double *__restrict__ partial)
{
    __shared__ double red[OPT_THREADS / 64];
    const int blk = blockIdx.x, i = opt_locate(t, blk);
    const int e = (blk - t.first[i]) * DLKA_OPTIM_CHUNK, len = min(t.count[i] - e, DLKA_OPTIM_CHUNK);
    const float *g = t.g[i] + e;
    const double acc = opt_aligned(g, nullptr, nullptr) ? opt_sumsq<true>(g, len) : opt_sumsq<false>(g, len);
    const double s = opt_block_sum(acc, red);
    if (threadIdx.x == 0) partial[(long)t.chunk_base + blk] = s;
}

__global__ __launch_bounds__(OPT_THREADS) void dlka_optim_norm_finish_kernel(const double *__restrict__ partial, int chunks, float *__restrict__ norm_out)
{
    __shared__ double red[OPT_THREADS / 64];
    double acc = 0.0;
    for (int c = threadIdx.x; c < chunks; c += OPT_THREADS) acc += partial[c];
    const double s = opt_block_sum(acc, red);
    if (threadIdx.x == 0) norm_out[0] = (float)sqrt(s);
}

template <bool VEC> __device__ __forceinline__ void opt_scale_chunk(float *__restrict__ g, int len, float coef)
{
#pragma unroll
    for (int j = 0; j < OPT_ITERS; ++j) {
        const int e0 = (j * OPT_THREADS + (int)threadIdx.x) * OPT_VEC;
        if (VEC && e0 + OPT_VEC <= len) {
            f32x4 q = act_load4(g, e0);
#pragma unroll
            for (int e = 0; e < OPT_VEC; ++e) q[e] = q[e] * coef;
            act_store4(g, e0, q);
        } else {
#pragma unroll
            for (int e = 0; e < OPT_VEC; ++e)
                if (e0 + e < len) g[e0 + e] = g[e0 + e] * coef;
        }
    }
}

__global__ __launch_bounds__(OPT_THREADS) void dlka_optim_scale_kernel(const OptimTable t, const float *__restrict__ norm_dev, float max_norm)
{
    const int blk = blockIdx.x, i = opt_locate(t, blk);
    const int e = (blk - t.first[i]) * DLKA_OPTIM_CHUNK, len = min(t.count[i] - e, DLKA_OPTIM_CHUNK);
    float *g = t.g[i] + e;
    const float coef = opt_clip_coef(norm_dev[0], max_norm);
    if (opt_aligned(g, nullptr, nullptr)) opt_scale_chunk<true>(g, len, coef); else opt_scale_chunk<false>(g, len, coef);
}

template <bool MOM> __device__ __forceinline__ void opt_sgd_elem(float &p, float g, float &b, float coef, float lr, const SgdArgs &a)
{
    if (a.clip) g = g * coef;
    const float d = a.weight_decay != 0.f ? g + a.weight_decay * p : g;
    float u = d;
    if (MOM) {
        b = a.momentum * b + d;
        u = a.nesterov ? d + a.momentum * b : b;
    }
    p = p - lr * u;
}

template <bool VEC, bool MOM>
__device__ __forceinline__ void opt_sgd_chunk(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ b, int len, float coef, float lr,
                                              const SgdArgs &a)
{
    if (VEC && len == DLKA_OPTIM_CHUNK) {   // a whole chunk: every load is issued before the first use
        f32x4 pv[OPT_ITERS], gv[OPT_ITERS], bv[OPT_ITERS];
#pragma unroll
        for (int j = 0; j < OPT_ITERS; ++j) {
            const int e0 = (j * OPT_THREADS + (int)threadIdx.x) * OPT_VEC;
            pv[j] = act_load4(p, e0);
            gv[j] = act_load4(g, e0);
            if (MOM) bv[j] = act_load4(b, e0);
        }
#pragma unroll
        for (int j = 0; j < OPT_ITERS; ++j) {
            const int e0 = (j * OPT_THREADS + (int)threadIdx.x) * OPT_VEC;
#pragma unroll
            for (int e = 0; e < OPT_VEC; ++e) {
                float pe = pv[j][e], be = MOM ? bv[j][e] : 0.f;
                opt_sgd_elem<MOM>(pe, gv[j][e], be, coef, lr, a);
                pv[j][e] = pe;
                if (MOM) bv[j][e] = be;
            }
            act_store4(p, e0, pv[j]);
            if (MOM) act_store4(b, e0, bv[j]);
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < OPT_ITERS; ++j) {
        const int e0 = (j * OPT_THREADS + (int)threadIdx.x) * OPT_VEC;
        if (VEC && e0 + OPT_VEC <= len) {
            f32x4 pv = act_load4(p, e0), bv = pv;
            const f32x4 gv = act_load4(g, e0);
            if (MOM) bv = act_load4(b, e0);
#pragma unroll
            for (int e = 0; e < OPT_VEC; ++e) {
                float pe = pv[e], be = bv[e];
                opt_sgd_elem<MOM>(pe, gv[e], be, coef, lr, a);
                pv[e] = pe;
                bv[e] = be;
            }
            act_store4(p, e0, pv);
            if (MOM) act_store4(b, e0, bv);
        } else {
#pragma unroll
            for (int e = 0; e < OPT_VEC; ++e) {
                if (e0 + e < len) {
                    float pe = p[e0 + e], be = MOM ? b[e0 + e] : 0.f;
                    opt_sgd_elem<MOM>(pe, g[e0 + e], be, coef, lr, a);
                    p[e0 + e] = pe;
                    if (MOM) b[e0 + e] = be;
                }
            }
        }
    }
}

template <bool MOM>
__global__ __launch_bounds__(OPT_THREADS) void dlka_optim_sgd_kernel(const OptimTable t, const SgdArgs a, const float *__restrict__ lr_dev,
                                                                     const float *__restrict__ norm_dev)
{
    const int blk = blockIdx.x, i = opt_locate(t, blk);
    const int e = (blk - t.first[i]) * DLKA_OPTIM_CHUNK, len = min(t.count[i] - e, DLKA_OPTIM_CHUNK);
    float *p = t.p[i] + e;
    const float *g = t.g[i] + e;
    float *b = MOM ? t.b[i] + e : nullptr;
    const float lr = lr_dev[a.lr_index];
    const float coef = a.clip ? opt_clip_coef(norm_dev[0], a.max_norm) : 1.f;
    if (opt_aligned(p, g, b)) opt_sgd_chunk<true, MOM>(p, g, b, len, coef, lr, a); else opt_sgd_chunk<false, MOM>(p, g, b, len, coef, lr, a);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------
// The refusals every entry shares, in the pipeline's order: NULL, shape, dtype, size.  other_null: a required pointer of the entry's own is
// missing.  *chunks: the chunk total of the list.  An empty list (n == 0) is DLKA_OK whatever else is passed: the caller launches nothing.
static int opt_check(const void *const *tables[], int n_tables, bool other_null, const int64_t *counts, int64_t n, int dtype, long *chunks)
{
    *chunks = 0;
    if (n == 0) return DLKA_OK;
    if (!counts || other_null) return DLKA_ERR_NULL;
    for (int k = 0; k < n_tables; ++k)
        if (!tables[k]) return DLKA_ERR_NULL;
    if (n < 0) return DLKA_ERR_SHAPE;
    for (int64_t i = 0; i < n; ++i)
        if (counts[i] < 0) return DLKA_ERR_SHAPE;
    if (dtype != DLKA_F32) return DLKA_ERR_DTYPE;
    if (n > 0x7fffffffL) return DLKA_ERR_UNSUPPORTED;
    for (int64_t i = 0; i < n; ++i) {
        if (counts[i] > 0x7fffffffL) return DLKA_ERR_UNSUPPORTED;
        *chunks += cdivl((long)counts[i], DLKA_OPTIM_CHUNK);
        if (*chunks > 0x7fffffffL) return DLKA_ERR_UNSUPPORTED;
    }
    for (int64_t i = 0; i < n; ++i)   // a tensor with elements has an address in every table
        for (int k = 0; k < n_tables; ++k)
            if (counts[i] > 0 && !tables[k][i]) return DLKA_ERR_NULL;
    return DLKA_OK;
}

// Cuts the list into tables and calls launch(table, grid) for every table that owns a chunk.
template <class Launch>
static int opt_walk(const void *const *p, const void *const *g, const void *const *b, const int64_t *counts, long n, Launch &&launch)
{
    long base = 0;
    for (long i0 = 0; i0 < n; i0 += DLKA_OPTIM_TENSORS_PER_LAUNCH) {
        OptimTable t = {};
        t.n = (int)(n - i0 < DLKA_OPTIM_TENSORS_PER_LAUNCH ? n - i0 : DLKA_OPTIM_TENSORS_PER_LAUNCH);
        t.chunk_base = (int)base;
        long grid = 0;
        for (int k = 0; k < t.n; ++k) {
            t.first[k] = (int)grid;
            t.count[k] = (int)counts[i0 + k];
            t.p[k] = p ? (float *)p[i0 + k] : nullptr;
            t.g[k] = g ? (float *)g[i0 + k] : nullptr;
            t.b[k] = b ? (float *)b[i0 + k] : nullptr;
            grid += cdivl((long)counts[i0 + k], DLKA_OPTIM_CHUNK);
        }
        for (int k = t.n; k <= DLKA_OPTIM_TENSORS_PER_LAUNCH; ++k) t.first[k] = (int)grid;
        if (grid == 0) continue;
        g_optim_launches.add();
        launch(t, dim3((unsigned)grid));
        DLKA_CHECK_LAUNCH();
        base += grid;
    }
    return DLKA_OK;
}

}  // namespace dlka

using namespace dlka;

extern "C" size_t dlka_optim_workspace_bytes(const int64_t *counts, int64_t n)
{
    long chunks = 0;
    if (n <= 0 || opt_check(nullptr, 0, false, counts, n, DLKA_F32, &chunks) != DLKA_OK) return 0;
    return (size_t)(chunks > 0 ? chunks : 1) * sizeof(double);
}

extern "C" int dlka_optim_grad_norm(const void *const *grads, const int64_t *counts, int64_t n, int dtype, void *workspace, size_t workspace_bytes,
                                    float *norm_out, void *stream)
{
    long chunks = 0;
    const void *const *tables[] = {grads};
    const int rc = opt_check(tables, 1, !norm_out, counts, n, dtype, &chunks);
    if (rc != DLKA_OK || n == 0) return rc;
    if (!workspace || ((uintptr_t)workspace & 7) != 0 || workspace_bytes < dlka_optim_workspace_bytes(counts, n)) return DLKA_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double *partial = (double *)workspace;
    const int rw = opt_walk(nullptr, grads, nullptr, counts, (long)n, [&](const OptimTable &t, dim3 grid) {
        DLKA_LAUNCH(dlka_optim_sumsq_kernel, grid, dim3(OPT_THREADS), 0, st, t, partial);
    });
    if (rw != DLKA_OK) return rw;
    g_optim_launches.add();
    DLKA_LAUNCH(dlka_optim_norm_finish_kernel, dim3(1), dim3(OPT_THREADS), 0, st, (const double *)partial, (int)chunks, norm_out);
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}

extern "C" int dlka_optim_scale(void *const *grads, const int64_t *counts, int64_t n, int dtype, const float *norm_dev, float max_norm, void *stream)
{
    long chunks = 0;
    const void *const *tables[] = {grads};
    const int rc = opt_check(tables, 1, !norm_dev, counts, n, dtype, &chunks);
    if (rc != DLKA_OK || n == 0) return rc;
    hipStream_t st = (hipStream_t)stream;
    return opt_walk(nullptr, grads, nullptr, counts, (long)n, [&](const OptimTable &t, dim3 grid) {
        DLKA_LAUNCH(dlka_optim_scale_kernel, grid, dim3(OPT_THREADS), 0, st, t, norm_dev, max_norm);
    });
}

extern "C" int dlka_optim_sgd_step(void *const *params, const void *const *grads, void *const *bufs, const int64_t *counts, const dlka_optim_desc *d,
                                   const float *lr_dev, const float *norm_dev, void *stream)
{
    if (!d) return DLKA_ERR_NULL;
    long chunks = 0;
    const void *const *tables[] = {params, grads, bufs};
    const int rc = opt_check(tables, d->has_momentum ? 3 : 2, !lr_dev || (d->clip && !norm_dev) || d->lr_index < 0, counts, d->n_tensors, d->dtype, &chunks);
    if (rc != DLKA_OK || d->n_tensors == 0) return rc;
    SgdArgs a = {};
    a.momentum = d->momentum; a.weight_decay = d->weight_decay; a.max_norm = d->max_norm;
    a.nesterov = d->nesterov; a.clip = d->clip; a.lr_index = d->lr_index;
    hipStream_t st = (hipStream_t)stream;
    return opt_walk(params, grads, d->has_momentum ? bufs : nullptr, counts, (long)d->n_tensors, [&](const OptimTable &t, dim3 grid) {
        if (d->has_momentum) DLKA_LAUNCH(dlka_optim_sgd_kernel<true>, grid, dim3(OPT_THREADS), 0, st, t, a, lr_dev, norm_dev);
        else DLKA_LAUNCH(dlka_optim_sgd_kernel<false>, grid, dim3(OPT_THREADS), 0, st, t, a, lr_dev, norm_dev);
    });
}
