// Resampling of class probabilities, images and label maps between the network's grid and the case's own grid (include/dlka.h:
// dlka_resample_*): what resample_data_or_seg (3D/d_lka_former/preprocessing/preprocessing.py:112-201) computes in float64 on one host core,
// channel by channel and slice by slice, for save_segmentation_nifti_from_softmax (inference/segmentation_export.py:73-137) and resample_patient
// (preprocessing.py:38-109).
//
// Every axis has a TABLE, built by the caller in float64 and rounded once: per output index the source cells and their weights under the map
// src = (i + 0.5) * n_in / n_out - 0.5 (skimage.transform.resize / scipy.ndimage.zoom(grid_mode=True); preprocessing.py:163-178 for the z step).
// Order 0 is one tap of weight 1, order 1 two taps (coordinate clamped to the array first: mode 'edge' / 'nearest'), order 3 four taps on
// prefiltered coefficients.  The kernels know taps and weights, not orders, so "in-plane linear with nearest z" (the trainers' export), full
// trilinear and "linear z" are one piece of arithmetic with 1 or 2 taps per axis.
//
//   argmax    (a) the hot path: a lane owns RS_VPT output voxels that are neighbours along the contiguous axis, walks the C classes with the
//             running maximum (first maximum wins, as numpy.argmax) in registers and stores RS_VPT label bytes; the resampled probabilities are
//             never written.  The source window of a class is left to L1/L2: neighbouring lanes read neighbouring source cells, and when the
//             grid is refined every source cell is read by several lanes of the same workgroup.
//   linear    (b) the same arithmetic (rs_lerp3, the same instruction sequence: the fused label map equals the argmax of this kernel's output bit
//             for bit), every channel written.
//   spline    (c) order 3, float64 throughout: separable 4-tap evaluation on the B-spline coefficients of the padded channel (cl_spline.hip
//             prepares them), clip to the input's range; only the caller rounds to the output dtype.
//   labels    (d) is_seg: the per-label passes of resize_segmentation (one resize of the indicator per label, ascending, later labels overwrite)
//             collapse into one visit of the up to 8 source cells: the weight of a label is the sum of the weights of the cells that hold it,
//             and the largest label whose weight passes the threshold wins; none: 0.
//
// No atomics, no reduction across lanes: every output cell is computed by one lane from the inputs alone, so two runs give the same bits.
#include "cl_resample.h"

DLKA_LAUNCH_COUNTER(g_rs_launches, dlka_resample_launch_count)   // cl_spline.hip's launches count here too

namespace dlka {

#define RS_THREADS 256
#define RS_VPT 4                          // output voxels per lane along the contiguous axis in the argmax / linear kernels

struct RsArgs {
    int C;
    int in[3], out[3], taps[3];
    long in_cells, out_cells;
    int off[3];                           // start of the axis' rows in the tables, in output indices
};

// Nested interpolation, axis 0 outermost.  Contraction is off so that every kernel that calls this rounds alike.
template <typename T>
__device__ __forceinline__ T rs_lerp3(const T *p, long sd, long sh, int n0, int n1, int n2, const int *i0, const T *w0, const int *i1,
                                      const T *w1, const int *i2, const T *w2)
{
#pragma clang fp contract(off)
    T acc0 = (T)0;
    for (int a = 0; a < n0; ++a) {
        const T *pa = p + (long)i0[a] * sd;
        T acc1 = (T)0;
        for (int b = 0; b < n1; ++b) {
            const T *pb = pa + (long)i1[b] * sh;
            T acc2 = (T)0;
            for (int c = 0; c < n2; ++c) acc2 = acc2 + w2[c] * pb[i2[c]];
            acc1 = acc1 + w1[b] * acc2;
        }
        acc0 = acc0 + w0[a] * acc1;
    }
    return acc0;
}

// What a lane of the argmax / linear kernels knows about its RS_VPT voxels.
template <typename T>
struct RsLane {
    int oz, oy, ox0, nv;
    int i0[2], i1[2], i2[RS_VPT][2];
    T w0[2], w1[2], w2[RS_VPT][2];
};

template <typename T>
__device__ __forceinline__ bool rs_lane(const RsArgs &a, const int *idx, const double *w, RsLane<T> &l)
{
    RowQuad q;
    if (!row_quad<RS_VPT, RS_THREADS>((long)a.out[0] * a.out[1], a.out[2], q)) return false;
    l.ox0 = q.x0;
    l.oy = (int)(q.row % a.out[1]);
    l.oz = (int)(q.row / a.out[1]);
    l.nv = q.nv;
    for (int k = 0; k < 2; ++k) {
        l.i0[k] = idx[2 * (a.off[0] + l.oz) + k];
        l.w0[k] = (T)w[2 * (a.off[0] + l.oz) + k];
        l.i1[k] = idx[2 * (a.off[1] + l.oy) + k];
        l.w1[k] = (T)w[2 * (a.off[1] + l.oy) + k];
    }
    for (int v = 0; v < RS_VPT; ++v) {
        const int ox = min(l.ox0 + v, a.out[2] - 1);
        for (int k = 0; k < 2; ++k) {
            l.i2[v][k] = idx[2 * (a.off[2] + ox) + k];
            l.w2[v][k] = (T)w[2 * (a.off[2] + ox) + k];
        }
    }
    return true;
}

// MODE 0: taps per axis from the description; 1: (1, 2, 2), in-plane linear with nearest z; 2: (2, 2, 2).
template <typename T, int MODE>
__global__ void __launch_bounds__(RS_THREADS) dlka_resample_argmax_kernel(RsArgs a, const T *x, unsigned char *y, const int *idx,
                                                                             const double *w, const int *region)
{
    RsLane<T> l;
    if (!rs_lane(a, idx, w, l)) return;
    const int n0 = MODE == 1 ? 1 : MODE == 2 ? 2 : a.taps[0];
    const int n1 = MODE ? 2 : a.taps[1], n2 = MODE ? 2 : a.taps[2];
    const long sh = a.in[2], sd = (long)a.in[1] * a.in[2];
    T best[RS_VPT];
    int lab[RS_VPT];
    for (int v = 0; v < RS_VPT; ++v) {
        best[v] = (T)0;
        lab[v] = 0;
    }
    for (int c = 0; c < a.C; ++c) {
        const T *p = x + (long)c * a.in_cells;
        const int rc = region ? region[c] : c;
        for (int v = 0; v < RS_VPT; ++v) {
            const T val = rs_lerp3(p, sd, sh, n0, n1, n2, l.i0, l.w0, l.i1, l.w1, l.i2[v], l.w2[v]);
            if (region) {
                if (val > (T)0.5) lab[v] = rc;             // segmentation_export.py:123-124: later regions overwrite
            } else if (c == 0 || val > best[v]) {          // numpy.argmax: the first maximum
                best[v] = val;
                lab[v] = c;
            }
        }
    }
    unsigned char *row = y + ((long)l.oz * a.out[1] + l.oy) * a.out[2] + l.ox0;
    if (l.nv == RS_VPT && (a.out[2] & 3) == 0) {
        *reinterpret_cast<unsigned *>(row) = (unsigned)(lab[0] & 255) | ((unsigned)(lab[1] & 255) << 8) | ((unsigned)(lab[2] & 255) << 16) |
                                             ((unsigned)(lab[3] & 255) << 24);
    } else {
        for (int v = 0; v < l.nv; ++v) row[v] = (unsigned char)lab[v];
    }
}

template <typename T>
__global__ void __launch_bounds__(RS_THREADS) dlka_resample_linear_kernel(RsArgs a, const T *x, T *y, const int *idx, const double *w)
{
    RsLane<T> l;
    if (!rs_lane(a, idx, w, l)) return;
    const long sh = a.in[2], sd = (long)a.in[1] * a.in[2];
    const long o = ((long)l.oz * a.out[1] + l.oy) * a.out[2] + l.ox0;
    for (int c = 0; c < a.C; ++c) {
        const T *p = x + (long)c * a.in_cells;
        for (int v = 0; v < l.nv; ++v)
            y[(long)c * a.out_cells + o + v] = rs_lerp3(p, sd, sh, a.taps[0], a.taps[1], a.taps[2], l.i0, l.w0, l.i1, l.w1, l.i2[v], l.w2[v]);
    }
}

// (d) one lane per output cell and channel.  The weight of a cell is ((1 * w0) * w1) * w2 and a label's weights are added in raster order of
// the cells, as scipy's map_coordinates evaluates the label's indicator.  strict: the reference's z step, round(.) > 0.5, which is "> 0.5"
// (numpy rounds 0.5 to 0); otherwise resize_segmentation's ">= 0.5".
__global__ void __launch_bounds__(RS_THREADS) dlka_resample_labels_kernel(RsArgs a, const int *seg, int *out, const int *idx, const double *w,
                                                                             int strict)
{
#pragma clang fp contract(off)
    const long q = (long)blockIdx.x * RS_THREADS + threadIdx.x;
    if (q >= a.C * a.out_cells) return;
    const long cell = q % a.out_cells;
    const int *p = seg + (q / a.out_cells) * a.in_cells;
    const int ox = (int)(cell % a.out[2]);
    const int oy = (int)((cell / a.out[2]) % a.out[1]);
    const int oz = (int)(cell / ((long)a.out[2] * a.out[1]));
    const int r0 = 2 * (a.off[0] + oz), r1 = 2 * (a.off[1] + oy), r2 = 2 * (a.off[2] + ox);
    int lab[8];
    double wt[8];
    int n = 0;
    for (int k0 = 0; k0 < a.taps[0]; ++k0)
        for (int k1 = 0; k1 < a.taps[1]; ++k1)
            for (int k2 = 0; k2 < a.taps[2]; ++k2) {
                lab[n] = p[((long)idx[r0 + k0] * a.in[1] + idx[r1 + k1]) * a.in[2] + idx[r2 + k2]];
                wt[n] = ((1.0 * w[r0 + k0]) * w[r1 + k1]) * w[r2 + k2];
                ++n;
            }
    bool found = false;
    int res = 0;
    for (int k = 0; k < n; ++k) {
        bool first = true;
        for (int j = 0; j < k; ++j) first = first && lab[j] != lab[k];
        if (!first) continue;
        double s = 0.0;
        for (int j = k; j < n; ++j)
            if (lab[j] == lab[k]) s = s + wt[j];
        if ((strict ? s > 0.5 : s >= 0.5) && (!found || lab[k] > res)) {
            found = true;
            res = lab[k];
        }
    }
    out[q] = res;
}

// ---- (c) order 3 ---------------------------------------------------------------------------------------------------------------------------
// Separable evaluation on the coefficients: per axis taps[ax] (1 or 4) cells from start[] with the weights w4[], then the clip to [lo, hi] of
// the volume (clip_axis < 0) or of the slice along clip_axis.
__global__ void __launch_bounds__(RS_THREADS) dlka_resample_spline_eval_kernel(RsArgs a, const double *coef, double *y, const int *start,
                                                                                  const double *w4, const double *lo, const double *hi,
                                                                                  int clip_axis)
{
#pragma clang fp contract(off)
    const long q = (long)blockIdx.x * RS_THREADS + threadIdx.x;
    if (q >= a.out_cells) return;
    int o[3];
    o[2] = (int)(q % a.out[2]);
    o[1] = (int)((q / a.out[2]) % a.out[1]);
    o[0] = (int)(q / ((long)a.out[2] * a.out[1]));
    const int s0 = start[a.off[0] + o[0]], s1 = start[a.off[1] + o[1]], s2 = start[a.off[2] + o[2]];
    const double *w0 = w4 + 4 * (a.off[0] + o[0]), *w1 = w4 + 4 * (a.off[1] + o[1]), *w2 = w4 + 4 * (a.off[2] + o[2]);
    double acc0 = 0.0;
    for (int k0 = 0; k0 < a.taps[0]; ++k0) {
        double acc1 = 0.0;
        for (int k1 = 0; k1 < a.taps[1]; ++k1) {
            const double *row = coef + ((long)(s0 + k0) * a.in[1] + (s1 + k1)) * a.in[2] + s2;
            double acc2 = 0.0;
            for (int k2 = 0; k2 < a.taps[2]; ++k2) acc2 = acc2 + w2[k2] * row[k2];
            acc1 = acc1 + w1[k1] * acc2;
        }
        acc0 = acc0 + w0[k0] * acc1;
    }
    const int s = clip_axis < 0 ? 0 : o[clip_axis];
    y[q] = fmin(fmax(acc0, lo[s]), hi[s]);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
static int rs_check(const dlka_resample_desc *d, int tap_hi, RsArgs *a)
{
    if (!d) return DLKA_ERR_NULL;
    if (d->C < 1) return DLKA_ERR_SHAPE;
    long ic = 1, oc = 1;
    const int rc = check_extents(3, {{d->in, 0x7fffffffL, a->in, &ic, nullptr}, {d->out, 0x7fffffffL, a->out, &oc, nullptr}},
                                 [&](int ax) { return d->taps[ax] != 1 && d->taps[ax] != tap_hi ? (int)DLKA_ERR_UNSUPPORTED : (int)DLKA_OK; });
    if (rc != DLKA_OK) return rc;
    long off = 0;
    for (int ax = 0; ax < 3; ++ax) {
        a->taps[ax] = d->taps[ax];
        a->off[ax] = (int)off;
        off += d->out[ax];
    }
    a->C = d->C;
    a->in_cells = ic;
    a->out_cells = oc;
    return DLKA_OK;
}

static unsigned rs_lane_blocks(const RsArgs &a) { return (unsigned)row_quad_blocks((long)a.out[0] * a.out[1], a.out[2], RS_VPT, RS_THREADS); }

}  // namespace dlka

using namespace dlka;

extern "C" int dlka_resample_argmax(const void *x, uint8_t *labels, const dlka_resample_desc *d, const int32_t *idx, const double *w,
                                    const int32_t *region_class, void *stream)
{
    RsArgs a;
    const int rc = rs_check(d, 2, &a);
    if (rc != DLKA_OK) return rc;
    if (!x || !labels || !idx || !w) return DLKA_ERR_NULL;
    return dispatch_storage<ST_F32 | ST_F64>(d->dtype, [&](auto t) -> int {
        using T = DLKA_T(t);
        if (d->C > 256) return DLKA_ERR_UNSUPPORTED;   // a label is one byte
        g_rs_launches.add();
        // kernel MODE 1: taps (1, 2, 2); 2: (2, 2, 2); 0: anything else
        const int mode = a.taps[1] == 2 && a.taps[2] == 2 ? a.taps[0] : 0;
        dispatch_int<0, 1, 2>(mode, [&](auto m) {
            DLKA_LAUNCH((dlka_resample_argmax_kernel<T, DLKA_V(m)>), dim3(rs_lane_blocks(a)), dim3(RS_THREADS), 0, (hipStream_t)stream, a,
                        (const T *)x, labels, idx, w, region_class);
        });
        DLKA_CHECK_LAUNCH();
        return DLKA_OK;
    });
}

extern "C" int dlka_resample_linear(const void *x, void *y, const dlka_resample_desc *d, const int32_t *idx, const double *w, void *stream)
{
    RsArgs a;
    const int rc = rs_check(d, 2, &a);
    if (rc != DLKA_OK) return rc;
    if (!x || !y || !idx || !w) return DLKA_ERR_NULL;
    if (x == y) return DLKA_ERR_UNSUPPORTED;
    return dispatch_storage<ST_F32 | ST_F64>(d->dtype, [&](auto t) -> int {
        using T = DLKA_T(t);
        g_rs_launches.add();
        DLKA_LAUNCH(dlka_resample_linear_kernel<T>, dim3(rs_lane_blocks(a)), dim3(RS_THREADS), 0, (hipStream_t)stream, a, (const T *)x, (T *)y,
                    idx, w);
        DLKA_CHECK_LAUNCH();
        return DLKA_OK;
    });
}

extern "C" int dlka_resample_labels(const int32_t *seg, int32_t *out, const dlka_resample_desc *d, const int32_t *idx, const double *w,
                                    int strict, void *stream)
{
    RsArgs a;
    const int rc = rs_check(d, 2, &a);
    if (rc != DLKA_OK) return rc;
    if (!seg || !out || !idx || !w) return DLKA_ERR_NULL;
    if (seg == out) return DLKA_ERR_UNSUPPORTED;
    if ((long)a.C * a.out_cells > 0x7fffffffL) return DLKA_ERR_UNSUPPORTED;
    g_rs_launches.add();
    DLKA_LAUNCH(dlka_resample_labels_kernel, dim3((unsigned)cdivl((long)a.C * a.out_cells, RS_THREADS)), dim3(RS_THREADS), 0,
                (hipStream_t)stream, a, seg, out, idx, w, strict);
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}

extern "C" int dlka_resample_spline_eval(const double *coef, double *y, const dlka_resample_desc *d, const int32_t *start, const double *w4,
                                         const double *lo, const double *hi, int clip_axis, void *stream)
{
    RsArgs a;
    const int rc = rs_check(d, 4, &a);
    if (rc != DLKA_OK) return rc;
    if (!coef || !y || !start || !w4 || !lo || !hi) return DLKA_ERR_NULL;
    if (clip_axis > 2) return DLKA_ERR_SHAPE;
    if (d->C != 1) return DLKA_ERR_UNSUPPORTED;
    g_rs_launches.add();
    DLKA_LAUNCH(dlka_resample_spline_eval_kernel, dim3((unsigned)cdivl(a.out_cells, RS_THREADS)), dim3(RS_THREADS), 0, (hipStream_t)stream, a,
                coef, y, start, w4, lo, hi, clip_axis);
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}
