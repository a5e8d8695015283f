// Host scaffolding and element access shared by the pipeline files (cl_tiles, cl_seg_loss, cl_surface_dist, cl_conn_comp, cl_resample,
// cl_spline, cl_augment, cl_preprocess, cl_zoom2d): every one is a set of extern "C" entries that turn 64-bit caller extents and a
// storage code into 32-bit kernel arguments and one template instantiation.  Nothing on the training path includes this.
#pragma once
#include <atomic>
#include <initializer_list>

#include "dlka_common.h"

namespace dlka {

// ---- element loads: any storage type as float64 (float32 from float / bf16_t: act_load1, dlka_common.h) ------------------------------------------
// STORES stay with their files because the int16 rule differs: zm_finish (cl_zoom2d.hip) rounds half away from zero, scipy's interpolation
// output; aug_st (cl_augment.hip) truncates towards zero, numpy's astype.
__device__ __forceinline__ double ld_f64(const double *p, long i) { return p[i]; }
__device__ __forceinline__ double ld_f64(const float *p, long i) { return (double)p[i]; }
__device__ __forceinline__ double ld_f64(const bf16_t *p, long i) { return (double)bf16_value(p[i].v); }
__device__ __forceinline__ double ld_f64(const int16_t *p, long i) { return (double)p[i]; }

// ---- storage code -> type, as dispatch_act (dlka_common.h): f(type_tag<T>{}) returns the entry's status --------------------------------------------
// The storage codes are dlka_dtype and int16, which the augmentation and the 2-D evaluator each name.
static_assert(DLKA_AUG_I16 == DLKA_ZOOM2D_I16 && DLKA_AUG_I16 == 3 && DLKA_F32 == 0 && DLKA_BF16 == 1 && DLKA_F64 == 2, "one storage code per type");
enum : unsigned { ST_F32 = 1u << DLKA_F32, ST_BF16 = 1u << DLKA_BF16, ST_F64 = 1u << DLKA_F64, ST_I16 = 1u << DLKA_AUG_I16, ST_ANY = 15u };
// Only the types in ALLOWED are instantiated; DLKA_ERR_DTYPE, and no call, for any other code.
template <unsigned ALLOWED, class F> int dispatch_storage(int code, F &&f)
{
    if constexpr ((ALLOWED & ST_F32) != 0) if (code == DLKA_F32) return f(type_tag<float>{});
    if constexpr ((ALLOWED & ST_BF16) != 0) if (code == DLKA_BF16) return f(type_tag<bf16_t>{});
    if constexpr ((ALLOWED & ST_F64) != 0) if (code == DLKA_F64) return f(type_tag<double>{});
    if constexpr ((ALLOWED & ST_I16) != 0) if (code == DLKA_AUG_I16) return f(type_tag<int16_t>{});
    return DLKA_ERR_DTYPE;
}

// label maps (dlka_sd_desc / dlka_cc_desc): bytes per label, 0 for an unknown code
inline int label_bytes(int code) { return code < DLKA_SD_U8 || code > DLKA_SD_I64 ? 0 : 1 << (code - DLKA_SD_U8); }
template <class F> int dispatch_label(int code, F &&f)
{
    switch (code) {
        case DLKA_SD_U8: return f(type_tag<uint8_t>{});
        case DLKA_SD_I16: return f(type_tag<int16_t>{});
        case DLKA_SD_I32: return f(type_tag<int32_t>{});
        case DLKA_SD_I64: return f(type_tag<int64_t>{});
        default: return DLKA_ERR_DTYPE;
    }
}

// ---- extents ----------------------------------------------------------------------------------------------------------------------------------------
// One group of per-axis extents of a description: n[ax] cells (1 .. limit), stored in ext[ax] as n[ax] + 2 pad[ax] (ext and pad may be
// NULL); *cells, which the caller initialises (1, or a batch count), is multiplied by every stored extent and must stay below 2^31.
struct Extents {
    const int64_t *n;
    long limit;
    int *ext;
    long *cells;
    const int64_t *pad;
};
// Axis by axis over all groups: an extent < 1 is DLKA_ERR_SHAPE; then axis(ax), the entry's own checks of that axis, may refuse; then an
// extent over its limit or a cell count over 2^31 - 1 is DLKA_ERR_UNSUPPORTED.  The first refusal in that order is the one returned.
template <class Axis> int check_extents(int axes, std::initializer_list<Extents> groups, Axis &&axis)
{
    for (int ax = 0; ax < axes; ++ax) {
        for (const Extents &g : groups)
            if (g.n[ax] < 1) return DLKA_ERR_SHAPE;
        const int rc = axis(ax);
        if (rc != DLKA_OK) return rc;
        for (const Extents &g : groups)
            if (g.n[ax] > g.limit) return DLKA_ERR_UNSUPPORTED;
        for (const Extents &g : groups) {
            const long e = g.n[ax] + (g.pad ? 2 * g.pad[ax] : 0);
            if (g.ext) g.ext[ax] = (int)e;
            if (*g.cells <= 0x7fffffffL) *g.cells *= e;      // (a count already over the bound is not multiplied further: no overflow)
            if (*g.cells > 0x7fffffffL) return DLKA_ERR_UNSUPPORTED;
        }
    }
    return DLKA_OK;
}
inline int check_extents(int axes, std::initializer_list<Extents> groups)
{
    return check_extents(axes, groups, [](int) { return (int)DLKA_OK; });
}

// ---- row quads: a lane owns up to VPT neighbours along W of one output row; the file splits `row` into its own outer indices ------------------------
struct RowQuad {
    long row;
    int x0, nv;
};
template <int VPT, int THREADS> __device__ __forceinline__ bool row_quad(long rows, int W, RowQuad &l)
{
    const int wq = cdiv(W, VPT);
    const long q = (long)blockIdx.x * THREADS + threadIdx.x;
    if (q >= rows * wq) return false;
    l.row = q / wq;
    l.x0 = (int)(q - l.row * wq) * VPT;
    l.nv = min(VPT, W - l.x0);
    return true;
}
// workgroups of such a launch: what the range check bounds and the grid uses
inline long row_quad_blocks(long rows, int W, int vpt, int threads) { return cdivl(rows * cdiv(W, vpt), threads); }

// ---- launch counters (include/dlka.h: dlka_*_launch_count, diagnostics) -----------------------------------------------------------------------------
struct LaunchCounter {
    std::atomic<long> n{0};
    void add(long k = 1) { n.fetch_add(k, std::memory_order_relaxed); }
};
// at file scope: the module's counter dlka::var and its reader
#define DLKA_LAUNCH_COUNTER(var, reader)                                                          \
    namespace dlka { LaunchCounter var; }                                                         \
    extern "C" long reader(void) { return dlka::var.n.load(std::memory_order_relaxed); }

}  // namespace dlka
