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
//   adam_step Adam / AdamW (Trainer_synapse.py:270-273: amsgrad; 2D/trainer_MaxViT_LKA.py:114) on a table of its own with five address columns:
//             a tick launch adds 1 to the listed tensors' float32 step counts in device memory and leaves 1 - beta1^t and sqrt(1 - beta2^t)
//             (float64, stored as float32) for the update launches, which visit every element once in torch.optim.Adam's order.
//
// Memory-bound: the norm reads the gradients once; the step reads p, g, buf and writes p, buf (Adam: reads p, g, m, v, vmax and writes all but
// g).  Contraction is off in this file: the two
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
    static constexpr int CAP = DLKA_OPTIM_TENSORS_PER_LAUNCH;
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
template <class Table> __device__ __forceinline__ int opt_locate(const Table &t, int blk)
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

// ---- Adam / AdamW ----------------------------------------------------------------------------------------------------------------------------------------
// Five address columns: fewer tensors a launch than OptimTable under the same argument budget.  tensor_base: the list index of record 0 (the
// slot of the tick's bias corrections).
struct AdamTable {
    static constexpr int CAP = DLKA_OPTIM_ADAM_TENSORS_PER_LAUNCH;
    int n, chunk_base, tensor_base;
    int first[DLKA_OPTIM_ADAM_TENSORS_PER_LAUNCH + 1];
    int count[DLKA_OPTIM_ADAM_TENSORS_PER_LAUNCH];
    float *p[DLKA_OPTIM_ADAM_TENSORS_PER_LAUNCH];
    float *g[DLKA_OPTIM_ADAM_TENSORS_PER_LAUNCH];
    float *m[DLKA_OPTIM_ADAM_TENSORS_PER_LAUNCH];
    float *v[DLKA_OPTIM_ADAM_TENSORS_PER_LAUNCH];
    float *vmax[DLKA_OPTIM_ADAM_TENSORS_PER_LAUNCH];
};
struct AdamArgs {
    float beta2, one_minus_beta1, one_minus_beta2, eps, weight_decay, max_norm;
    int decoupled, clip, lr_index;
};
static_assert(sizeof(AdamTable) + sizeof(AdamArgs) + 3 * sizeof(void *) <= 4096, "the kernel-argument budget");
struct AdamTickTable {
    int n, tensor_base;
    float *step[DLKA_OPTIM_ADAM_TICK_PER_LAUNCH];
};
static_assert(sizeof(AdamTickTable) + 2 * sizeof(double) + sizeof(void *) <= 4096, "the kernel-argument budget");

// t += 1 for every listed tensor, and the two bias corrections of the new t where the update's workgroups read them: the update itself writes
// no count, so every workgroup of a tensor sees the same t.
__global__ __launch_bounds__(OPT_THREADS) void dlka_optim_adam_tick_kernel(const AdamTickTable t, double beta1, double beta2, float *__restrict__ bias)
{
    for (int k = threadIdx.x; k < t.n; k += OPT_THREADS) {
        const float s = t.step[k][0] + 1.f;
        t.step[k][0] = s;
        bias[2 * (long)(t.tensor_base + k)] = (float)(1.0 - pow(beta1, (double)s));
        bias[2 * (long)(t.tensor_base + k) + 1] = (float)sqrt(1.0 - pow(beta2, (double)s));
    }
}

struct AdamLane {   // the same in every lane of a tensor
    float coef, decay, step_size, bc2_sqrt;
};

template <bool AMS> __device__ __forceinline__ void opt_adam_elem(float &p, float g, float &m, float &v, float &vm, const AdamLane &c, const AdamArgs &a)
{
    if (a.clip) g = g * c.coef;
    if (a.decoupled) p = p * c.decay;
    else if (a.weight_decay != 0.f) g = g + a.weight_decay * p;
    m = m + (g - m) * a.one_minus_beta1;
    v = a.beta2 * v + a.one_minus_beta2 * (g * g);
    float w = v;
    if (AMS) {
        vm = (v > vm || v != v) ? v : vm;   // torch.maximum: a NaN on either side stays
        w = vm;
    }
    const float denom = sqrtf(w) / c.bc2_sqrt + a.eps;
    p = p - (c.step_size * m) / denom;
}

// OPT_ADAM_GROUP sweeps of a whole chunk have their loads issued before the first use (all OPT_ITERS of them would hold 80 data registers
// with five arrays and halve the waves per SIMD; two keep the kernel at eight waves and still leave > 10 KB in flight per wave).
#define OPT_ADAM_GROUP 2
static_assert(OPT_ITERS % OPT_ADAM_GROUP == 0, "a chunk is a whole number of load groups");

template <bool VEC, bool AMS>
__device__ __forceinline__ void opt_adam_chunk(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
                                               float *__restrict__ vm, int len, const AdamLane &c, const AdamArgs &a)
{
    if (VEC && len == DLKA_OPTIM_CHUNK) {
#pragma unroll
        for (int j0 = 0; j0 < OPT_ITERS; j0 += OPT_ADAM_GROUP) {
            f32x4 pv[OPT_ADAM_GROUP], gv[OPT_ADAM_GROUP], mv[OPT_ADAM_GROUP], vv[OPT_ADAM_GROUP], xv[OPT_ADAM_GROUP];
#pragma unroll
            for (int j = 0; j < OPT_ADAM_GROUP; ++j) {
                const int e0 = ((j0 + j) * OPT_THREADS + (int)threadIdx.x) * OPT_VEC;
                pv[j] = act_load4(p, e0);
                gv[j] = act_load4(g, e0);
                mv[j] = act_load4(m, e0);
                vv[j] = act_load4(v, e0);
                if (AMS) xv[j] = act_load4(vm, e0);
            }
#pragma unroll
            for (int j = 0; j < OPT_ADAM_GROUP; ++j) {
                const int e0 = ((j0 + j) * OPT_THREADS + (int)threadIdx.x) * OPT_VEC;
#pragma unroll
                for (int e = 0; e < OPT_VEC; ++e) {
                    float pe = pv[j][e], me = mv[j][e], ve = vv[j][e], xe = AMS ? xv[j][e] : 0.f;
                    opt_adam_elem<AMS>(pe, gv[j][e], me, ve, xe, c, a);
                    pv[j][e] = pe;
                    mv[j][e] = me;
                    vv[j][e] = ve;
                    if (AMS) xv[j][e] = xe;
                }
                act_store4(p, e0, pv[j]);
                act_store4(m, e0, mv[j]);
                act_store4(v, e0, vv[j]);
                if (AMS) act_store4(vm, e0, xv[j]);
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < OPT_ITERS; ++j) {
        const int e0 = (j * OPT_THREADS + (int)threadIdx.x) * OPT_VEC;
        if (VEC && e0 + OPT_VEC <= len) {
            f32x4 pv = act_load4(p, e0), mv = act_load4(m, e0), vv = act_load4(v, e0), xv = pv;
            const f32x4 gv = act_load4(g, e0);
            if (AMS) xv = act_load4(vm, e0);
#pragma unroll
            for (int e = 0; e < OPT_VEC; ++e) {
                float pe = pv[e], me = mv[e], ve = vv[e], xe = AMS ? xv[e] : 0.f;
                opt_adam_elem<AMS>(pe, gv[e], me, ve, xe, c, a);
                pv[e] = pe;
                mv[e] = me;
                vv[e] = ve;
                xv[e] = xe;
            }
            act_store4(p, e0, pv);
            act_store4(m, e0, mv);
            act_store4(v, e0, vv);
            if (AMS) act_store4(vm, e0, xv);
        } else {
#pragma unroll
            for (int e = 0; e < OPT_VEC; ++e) {
                if (e0 + e < len) {
                    float pe = p[e0 + e], me = m[e0 + e], ve = v[e0 + e], xe = AMS ? vm[e0 + e] : 0.f;
                    opt_adam_elem<AMS>(pe, g[e0 + e], me, ve, xe, c, a);
                    p[e0 + e] = pe;
                    m[e0 + e] = me;
                    v[e0 + e] = ve;
                    if (AMS) vm[e0 + e] = xe;
                }
            }
        }
    }
}

template <bool AMS>
__global__ __launch_bounds__(OPT_THREADS) void dlka_optim_adam_kernel(const AdamTable t, const AdamArgs a, const float *__restrict__ lr_dev,
                                                                      const float *__restrict__ norm_dev, const float *__restrict__ bias)
{
    const int blk = blockIdx.x, i = opt_locate(t, blk);
    const int e = (blk - t.first[i]) * DLKA_OPTIM_CHUNK, len = min(t.count[i] - e, DLKA_OPTIM_CHUNK);
    float *p = t.p[i] + e, *m = t.m[i] + e, *v = t.v[i] + e;
    const float *g = t.g[i] + e;
    float *vm = AMS ? t.vmax[i] + e : nullptr;
    const float lr = lr_dev[a.lr_index];
    AdamLane c;
    c.coef = a.clip ? opt_clip_coef(norm_dev[0], a.max_norm) : 1.f;
    c.decay = 1.f - lr * a.weight_decay;
    c.step_size = lr / bias[2 * (long)(t.tensor_base + i)];
    c.bc2_sqrt = bias[2 * (long)(t.tensor_base + i) + 1];
    const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)vm) & 15) == 0);
    if (vec) opt_adam_chunk<true, AMS>(p, g, m, v, vm, len, c, a); else opt_adam_chunk<false, AMS>(p, g, m, v, vm, len, c, a);
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

// Cuts the list into tables of up to Table::CAP tensors -- fill(table, k, i) writes the addresses of list entry i into record k -- and calls
// launch(table, grid) for every table that owns a chunk.
template <class Table, class Fill, class Launch> static int opt_walk_tables(const int64_t *counts, long n, Fill &&fill, Launch &&launch)
{
    long base = 0;
    for (long i0 = 0; i0 < n; i0 += Table::CAP) {
        Table t = {};
        t.n = (int)(n - i0 < Table::CAP ? n - i0 : Table::CAP);
        t.chunk_base = (int)base;
        long grid = 0;
        for (int k = 0; k < t.n; ++k) {
            t.first[k] = (int)grid;
            t.count[k] = (int)counts[i0 + k];
            fill(t, k, i0 + k);
            grid += cdivl((long)counts[i0 + k], DLKA_OPTIM_CHUNK);
        }
        for (int k = t.n; k <= Table::CAP; ++k) t.first[k] = (int)grid;
        if (grid == 0) continue;
        g_optim_launches.add();
        launch(t, dim3((unsigned)grid));
        DLKA_CHECK_LAUNCH();
        base += grid;
    }
    return DLKA_OK;
}

template <class Launch>
static int opt_walk(const void *const *p, const void *const *g, const void *const *b, const int64_t *counts, long n, Launch &&launch)
{
    return opt_walk_tables<OptimTable>(counts, n, [&](OptimTable &t, int k, long i) {
        t.p[k] = p ? (float *)p[i] : nullptr;
        t.g[k] = g ? (float *)g[i] : nullptr;
        t.b[k] = b ? (float *)b[i] : nullptr;
    }, launch);
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

extern "C" size_t dlka_optim_adam_workspace_bytes(int64_t n_tensors)
{
    return n_tensors > 0 && n_tensors <= 0x7fffffffL ? (size_t)n_tensors * 2 * sizeof(float) : 0;
}

extern "C" int dlka_optim_adam_step(void *const *params, const void *const *grads, void *const *exp_avg, void *const *exp_avg_sq,
                                    void *const *max_exp_avg_sq, void *const *steps, const int64_t *counts, const dlka_optim_adam_desc *d,
                                    const float *lr_dev, const float *norm_dev, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!d) return DLKA_ERR_NULL;
    long chunks = 0;
    const long n = d->n_tensors;
    if (n == 0) return DLKA_OK;
    const void *const *tables[] = {params, grads, exp_avg, exp_avg_sq, steps, max_exp_avg_sq};
    if (!counts || !lr_dev || (d->clip && !norm_dev)) return DLKA_ERR_NULL;
    for (int k = 0; k < (d->amsgrad ? 6 : 5); ++k)
        if (!tables[k]) return DLKA_ERR_NULL;
    const bool bad = d->lr_index < 0 || !(d->beta1 >= 0.0 && d->beta1 < 1.0) || !(d->beta2 >= 0.0 && d->beta2 < 1.0) || !(d->eps >= 0.0) ||
                     !(d->weight_decay >= 0.0);
    if (n < 0 || bad) return DLKA_ERR_SHAPE;
    const void *const *elems[] = {params, grads, exp_avg, exp_avg_sq, max_exp_avg_sq};
    const int rc = opt_check(elems, d->amsgrad ? 5 : 4, false, counts, n, d->dtype, &chunks);
    if (rc != DLKA_OK) return rc;
    for (long i = 0; i < n; ++i)
        if (!steps[i]) return DLKA_ERR_NULL;
    if (!workspace || ((uintptr_t)workspace & 3) != 0 || workspace_bytes < dlka_optim_adam_workspace_bytes(n)) return DLKA_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float *bias = (float *)workspace;
    for (long i0 = 0; i0 < n; i0 += DLKA_OPTIM_ADAM_TICK_PER_LAUNCH) {
        AdamTickTable tt = {};
        tt.n = (int)(n - i0 < DLKA_OPTIM_ADAM_TICK_PER_LAUNCH ? n - i0 : DLKA_OPTIM_ADAM_TICK_PER_LAUNCH);
        tt.tensor_base = (int)i0;
        for (int k = 0; k < tt.n; ++k) tt.step[k] = (float *)steps[i0 + k];
        g_optim_launches.add();
        DLKA_LAUNCH(dlka_optim_adam_tick_kernel, dim3(1), dim3(OPT_THREADS), 0, st, tt, d->beta1, d->beta2, bias);
        DLKA_CHECK_LAUNCH();
    }
    AdamArgs a = {};
    a.beta2 = (float)d->beta2; a.one_minus_beta1 = (float)(1.0 - d->beta1); a.one_minus_beta2 = (float)(1.0 - d->beta2);
    a.eps = (float)d->eps; a.weight_decay = (float)d->weight_decay; a.max_norm = d->max_norm;
    a.decoupled = d->decoupled; a.clip = d->clip; a.lr_index = d->lr_index;
    const bool ams = d->amsgrad != 0;
    return opt_walk_tables<AdamTable>(counts, n, [&](AdamTable &t, int k, long i) {
        if (k == 0) t.tensor_base = (int)i;
        t.p[k] = (float *)params[i];
        t.g[k] = (float *)grads[i];
        t.m[k] = (float *)exp_avg[i];
        t.v[k] = (float *)exp_avg_sq[i];
        t.vmax[k] = ams ? (float *)max_exp_avg_sq[i] : nullptr;
    }, [&](const AdamTable &t, dim3 grid) {
        if (ams) DLKA_LAUNCH(dlka_optim_adam_kernel<true>, grid, dim3(OPT_THREADS), 0, st, t, a, lr_dev, norm_dev, (const float *)bias);
        else DLKA_LAUNCH(dlka_optim_adam_kernel<false>, grid, dim3(OPT_THREADS), 0, st, t, a, lr_dev, norm_dev, (const float *)bias);
    });
}
