// The 2-D evaluator's slice resampling (include/dlka.h: dlka_zoom2d_*): what test_single_volume (2D/utils.py:63-110) and the resize tail of
// Synapse_dataset.__getitem__ (2D/datasets/dataset_synapse.py:109-112) compute with scipy.ndimage.zoom on one host core, slice by slice:
// order 3 of a 512 x 512 slice to the patch size, ToTensor / Normalize, and after the network softmax, argmax, a copy to the host and the
// order-0 zoom of the label map back to 512 x 512.
//
// scipy.ndimage.zoom with its defaults (mode 'constant', cval 0, grid_mode False): output index k of an axis n -> m reads the source coordinate
// k * ((n - 1) / (m - 1)), and a coordinate < 0 or > n - 1 gives cval at every order.  The caller builds one TABLE per axis in float64 on the
// host (deformablelka_amd/inference2d.py), so the rounding of that product, including the pairs for which the last coordinate exceeds n - 1 by
// one ulp and the whole last row or column is 0 (512 -> 224), is scipy's and the kernels never form a coordinate.
//
//   spline    (a) a stack of slices through 4 x 4 taps on float64 B-spline coefficients (cl_spline.hip's 'mirror' prefilter along
//             axes 1 and 2 of the stack), or 2 x 2 taps on the raw values (order 1).  A lane owns ZM_VPT output pixels that are neighbours along
//             W, holds their column tables (mirrored tap indices and weights) in registers and walks ZM_ROWS output rows with them; the sum is
//             scipy's, t += (c * w_row) * w_col with the rows outermost, rounded once to float32, then optionally (v - mean) / std in float32 (one
//             IEEE subtraction, one IEEE division) and optionally rounded to bf16.  int16: scipy's round half away from zero, saturated.
//   nearest   (b) order 0: a gather of 1, 2, 4 or 8 byte elements through two index tables; outside: 0.
//   argmax    (c) the argmax over the K logit planes of a chunk of slices evaluated only at the source pixel the order-0 zoom back selects for
//             each output pixel, first maximum wins; a lane reuses its previous pixel's label when the source column repeats (2.3 x per axis for
//             224 -> 512) and stores its ZM_VPT label bytes as one 32-bit word.  The (N, h, w) label map is never written.
//
// No atomics, no reduction across lanes: every output cell is computed by one lane from the inputs alone, so two runs give the same bits.  Tap
// and source indices are mirrored / range-checked in the lane, so no table can make a kernel read outside its input.
#include "cl_pipeline.h"

DLKA_LAUNCH_COUNTER(g_zm_launches, dlka_zoom2d_launch_count)

namespace dlka {

#define ZM_THREADS 256
#define ZM_VPT 4                             // output pixels per lane along W
#define ZM_ROWS 4                            // output rows a lane of the spline kernel walks with its column tables in registers
#define ZM_COLS (64 * ZM_VPT)                // output columns of a workgroup of the spline kernel: one wave wide
#define ZM_TILE_ROWS ((ZM_THREADS / 64) * ZM_ROWS)

struct ZmArgs {
    int N, ih, iw, oh, ow;
    int ctiles, rtiles;                      // spline kernel: workgroups per output row / per slice column
    int K;                                   // argmax kernel: logit planes
    int normalize;
    float mean, std;
};

// ---- storage types (loads: cl_pipeline.h) -----------------------------------------------------------------------------------------------------
// The float64 sum of one pixel in its storage type.
__device__ __forceinline__ float zm_f32(double t, const ZmArgs &a)
{
#pragma clang fp contract(off)
    float v = (float)t;
    if (a.normalize) v = (v - a.mean) / a.std;
    return v;
}
__device__ __forceinline__ void zm_finish(float *o, double t, const ZmArgs &a) { *o = zm_f32(t, a); }
__device__ __forceinline__ void zm_finish(bf16_t *o, double t, const ZmArgs &a) { o->v = bf16_bits(zm_f32(t, a)); }
__device__ __forceinline__ void zm_finish(int16_t *o, double t, const ZmArgs &)
{
    t = t > 0.0 ? t + 0.5 : t - 0.5;         // (scipy's CASE_INTERP_OUT_INT; a NaN becomes 0)
    *o = t != t ? (int16_t)0 : (int16_t)(int)fmin(fmax(t, -32768.0), 32767.0);
}

// nv (<= ZM_VPT) neighbours of a row, as one store where the row allows it
template <typename T>
__device__ __forceinline__ void zm_store(T *row, const T *v, int nv, bool whole)
{
    if (whole && nv == ZM_VPT) {
        if constexpr (sizeof(T) == 1) {
            unsigned w;
            memcpy(&w, v, 4);
            *reinterpret_cast<unsigned *>(row) = w;
            return;
        }
        if constexpr (sizeof(T) == 2) {
            ActU2 w;
            memcpy(&w, v, 8);
            *reinterpret_cast<ActU2 *>(row) = w;
            return;
        }
        if constexpr (sizeof(T) == 4) {
            f32x4 w;
            memcpy(&w, v, 16);
            *reinterpret_cast<f32x4 *>(row) = w;
            return;
        }
    }
    for (int k = 0; k < nv; ++k) row[k] = v[k];
}

// scipy's 'mirror' extension of the coefficients (a tap beyond the slice under mode 'constant'); any i lands in [0, n).
__device__ __forceinline__ int zm_mirror(int i, int n)
{
    if (i >= 0 && i < n) return i;
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

// (a) one workgroup: ZM_COLS output columns x ZM_TILE_ROWS output rows of one slice; lanes 0..63 of every wave are the column quads.
template <typename S, typename O, int TAPS>
__global__ void __launch_bounds__(ZM_THREADS) dlka_zoom2d_spline_kernel(ZmArgs a, const S *src, O *y, const int *start, const double *w4)
{
#pragma clang fp contract(off)
    long b = (long)blockIdx.x;
    const int ct = (int)(b % a.ctiles);
    b /= a.ctiles;
    const int rt = (int)(b % a.rtiles);
    const int n = (int)(b / a.rtiles);
    const int ox0 = (ct * 64 + ((int)threadIdx.x & 63)) * ZM_VPT;
    if (n >= a.N || ox0 >= a.ow) return;
    const int nv = min(ZM_VPT, a.ow - ox0);
    bool cin[ZM_VPT];
    int ci[ZM_VPT][TAPS];
    double cw[ZM_VPT][TAPS];
    for (int v = 0; v < ZM_VPT; ++v) {
        const int ox = min(ox0 + v, a.ow - 1);
        const int s = start[a.oh + ox];
        cin[v] = s != DLKA_ZOOM2D_OUTSIDE;
        for (int k = 0; k < TAPS; ++k) {
            ci[v][k] = cin[v] ? zm_mirror(s + k, a.iw) : 0;
            cw[v][k] = w4[4 * (long)(a.oh + ox) + k];
        }
    }
    const S *p = src + (long)n * a.ih * a.iw;
    const bool whole = (a.ow % ZM_VPT) == 0;
    const int oy0 = (rt * (ZM_THREADS / 64) + ((int)threadIdx.x >> 6)) * ZM_ROWS;
    for (int r = 0; r < ZM_ROWS; ++r) {
        const int oy = oy0 + r;
        if (oy >= a.oh) break;
        const int s = start[oy];
        const bool rin = s != DLKA_ZOOM2D_OUTSIDE;
        long ro[TAPS];
        double rw[TAPS];
        for (int k = 0; k < TAPS; ++k) {
            ro[k] = rin ? (long)zm_mirror(s + k, a.ih) * a.iw : 0L;
            rw[k] = w4[4 * (long)oy + k];
        }
        O res[ZM_VPT];
        for (int v = 0; v < ZM_VPT; ++v) {
            double t = 0.0;                                    // cval
            if (rin && cin[v]) {
                for (int kr = 0; kr < TAPS; ++kr)
                    for (int kc = 0; kc < TAPS; ++kc) t = t + (ld_f64(p, ro[kr] + ci[v][kc]) * rw[kr]) * cw[v][kc];
            }
            zm_finish(&res[v], t, a);
        }
        zm_store(y + ((long)n * a.oh + oy) * a.ow + ox0, res, nv, whole);
    }
}

// What a lane of the nearest / argmax kernels owns: ZM_VPT neighbours of one output row.
struct ZmLane {
    int n, oy, ox0, nv;
};

__device__ __forceinline__ bool zm_lane(const ZmArgs &a, ZmLane &l)
{
    RowQuad q;
    if (!row_quad<ZM_VPT, ZM_THREADS>((long)a.N * a.oh, a.ow, q)) return false;
    l.ox0 = q.x0;
    l.oy = (int)(q.row % a.oh);
    l.n = (int)(q.row / a.oh);
    l.nv = q.nv;
    return true;
}

// (b) idx: oh source rows, then ow source columns; anything outside [0, extent) is "outside".
template <typename U>
__global__ void __launch_bounds__(ZM_THREADS) dlka_zoom2d_nearest_kernel(ZmArgs a, const U *x, U *y, const int *idx)
{
    ZmLane l;
    if (!zm_lane(a, l)) return;
    const int sr = idx[l.oy];
    const bool rin = (unsigned)sr < (unsigned)a.ih;
    const U *row = x + ((long)l.n * a.ih + (rin ? sr : 0)) * a.iw;
    U res[ZM_VPT];
    for (int v = 0; v < ZM_VPT; ++v) {
        const int sc = idx[a.oh + min(l.ox0 + v, a.ow - 1)];
        res[v] = (rin && (unsigned)sc < (unsigned)a.iw) ? row[sc] : (U)0;
    }
    zm_store(y + ((long)l.n * a.oh + l.oy) * a.ow + l.ox0, res, l.nv, (a.ow % ZM_VPT) == 0);
}

// (c) logits (N, K, ih, iw); labels (N, oh, ow) uint8.
template <typename T>
__global__ void __launch_bounds__(ZM_THREADS) dlka_zoom2d_argmax_kernel(ZmArgs a, const T *logits, uint8_t *y, const int *idx)
{
    ZmLane l;
    if (!zm_lane(a, l)) return;
    uint8_t res[ZM_VPT] = {0, 0, 0, 0};
    const int sr = idx[l.oy];
    if ((unsigned)sr < (unsigned)a.ih) {
        const long plane = (long)a.ih * a.iw;
        const T *p = logits + (long)l.n * a.K * plane + (long)sr * a.iw;
        int prev = -1;
        uint8_t prev_label = 0;
        for (int v = 0; v < l.nv; ++v) {
            const int sc = idx[a.oh + l.ox0 + v];
            if ((unsigned)sc >= (unsigned)a.iw) continue;      // outside: 0
            if (sc != prev) {
                float best = act_load1(p, sc);
                int lab = 0;
                for (int c = 1; c < a.K; ++c) {
                    const float val = act_load1(p, (long)c * plane + sc);
                    if (val > best) {                          // the first maximum
                        best = val;
                        lab = c;
                    }
                }
                prev = sc;
                prev_label = (uint8_t)lab;
            }
            res[v] = prev_label;
        }
    }
    zm_store(y + ((long)l.n * a.oh + l.oy) * a.ow + l.ox0, res, l.nv, (a.ow % ZM_VPT) == 0);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
static int zm_check(const dlka_zoom2d_desc *d, ZmArgs *a)
{
    if (!d) return DLKA_ERR_NULL;
    if (d->N < 1) return DLKA_ERR_SHAPE;
    long ic = d->N, oc = d->N;                // (an N over 2^31 - 1 is refused as a cell count, after the first axis' extents)
    int in[2], out[2];
    const int rc = check_extents(2, {{d->in, 0x3fffffffL, in, &ic, nullptr}, {d->out, 0x3fffffffL, out, &oc, nullptr}});
    if (rc != DLKA_OK) return rc;
    a->N = (int)d->N;
    a->ih = in[0];
    a->iw = in[1];
    a->oh = out[0];
    a->ow = out[1];
    a->ctiles = cdiv(a->ow, ZM_COLS);
    a->rtiles = cdiv(a->oh, ZM_TILE_ROWS);
    a->K = 1;
    a->normalize = d->normalize != 0;
    a->mean = d->mean;
    a->std = d->std;
    return DLKA_OK;
}

static unsigned zm_lane_blocks(const ZmArgs &a) { return (unsigned)row_quad_blocks((long)a.N * a.oh, a.ow, ZM_VPT, ZM_THREADS); }

}  // namespace dlka

using namespace dlka;

extern "C" int dlka_zoom2d_spline(const void *src, void *y, const dlka_zoom2d_desc *d, const int32_t *start, const double *w4, void *stream)
{
    ZmArgs a;
    const int rc = zm_check(d, &a);
    if (rc != DLKA_OK) return rc;
    if (!src || !y || !start || !w4) return DLKA_ERR_NULL;
    if (src == y) return DLKA_ERR_UNSUPPORTED;
    if ((long)a.N * a.rtiles * a.ctiles > 0x7fffffffL) return DLKA_ERR_UNSUPPORTED;
    const int in = d->in_dtype, out = d->out_dtype;
    if (d->taps == 4) {
        if (in != DLKA_F64 || (out != DLKA_F32 && out != DLKA_BF16 && out != DLKA_ZOOM2D_I16)) return DLKA_ERR_DTYPE;
    } else if (d->taps == 2) {
        const bool ok = (in == DLKA_F32 && (out == DLKA_F32 || out == DLKA_BF16)) || (in == DLKA_BF16 && out == DLKA_BF16) ||
                        (in == DLKA_ZOOM2D_I16 && out == DLKA_ZOOM2D_I16);
        if (!ok) return DLKA_ERR_DTYPE;
    } else {
        return DLKA_ERR_UNSUPPORTED;
    }
    if (a.normalize && (out == DLKA_ZOOM2D_I16 || !(d->std == d->std) || d->std == 0.f)) return DLKA_ERR_UNSUPPORTED;
    g_zm_launches.add();
    const dim3 grid((unsigned)((long)a.N * a.rtiles * a.ctiles)), block(ZM_THREADS);
    auto launch = [&](auto s, auto o, auto taps) -> int {
        using S = DLKA_T(s);
        using O = DLKA_T(o);
        DLKA_LAUNCH((dlka_zoom2d_spline_kernel<S, O, DLKA_V(taps)>), grid, block, 0, (hipStream_t)stream, a, (const S *)src, (O *)y, start, w4);
        DLKA_CHECK_LAUNCH();
        return DLKA_OK;
    };
    if (d->taps == 4) return dispatch_storage<ST_F32 | ST_BF16 | ST_I16>(out, [&](auto o) { return launch(type_tag<double>{}, o, int_c<4>{}); });
    return dispatch_storage<ST_F32 | ST_BF16 | ST_I16>(in, [&](auto s) {      // two taps: the output has the input's type, or float -> bf16
        if constexpr (std::is_same<DLKA_T(s), float>::value)
            if (out == DLKA_BF16) return launch(s, type_tag<bf16_t>{}, int_c<2>{});
        return launch(s, s, int_c<2>{});
    });
}

extern "C" int dlka_zoom2d_nearest(const void *x, void *y, const dlka_zoom2d_desc *d, int elem_bytes, const int32_t *idx, void *stream)
{
    ZmArgs a;
    const int rc = zm_check(d, &a);
    if (rc != DLKA_OK) return rc;
    if (!x || !y || !idx) return DLKA_ERR_NULL;
    if (x == y) return DLKA_ERR_UNSUPPORTED;
    // an element of 1, 2, 4 or 8 bytes moves as the unsigned integer of the label type of that size
    const int code = elem_bytes == 1 ? DLKA_SD_U8 : elem_bytes == 2 ? DLKA_SD_I16 : elem_bytes == 4 ? DLKA_SD_I32 : elem_bytes == 8 ? DLKA_SD_I64 : -1;
    return dispatch_label(code, [&](auto t) -> int {
        using U = std::make_unsigned_t<DLKA_T(t)>;
        g_zm_launches.add();
        DLKA_LAUNCH(dlka_zoom2d_nearest_kernel<U>, dim3(zm_lane_blocks(a)), dim3(ZM_THREADS), 0, (hipStream_t)stream, a, (const U *)x, (U *)y, idx);
        DLKA_CHECK_LAUNCH();
        return DLKA_OK;
    });
}

extern "C" int dlka_zoom2d_argmax(const void *logits, uint8_t *labels, const dlka_zoom2d_desc *d, int K, const int32_t *idx, void *stream)
{
    ZmArgs a;
    const int rc = zm_check(d, &a);
    if (rc != DLKA_OK) return rc;
    if (!logits || !labels || !idx) return DLKA_ERR_NULL;
    if (K < 1) return DLKA_ERR_SHAPE;
    if (K > DLKA_ZOOM2D_K_MAX) return DLKA_ERR_UNSUPPORTED;   // a label is one byte
    a.K = K;
    return dispatch_storage<ST_F32 | ST_BF16>(d->in_dtype, [&](auto t) -> int {
        using T = DLKA_T(t);
        g_zm_launches.add();
        DLKA_LAUNCH(dlka_zoom2d_argmax_kernel<T>, dim3(zm_lane_blocks(a)), dim3(ZM_THREADS), 0, (hipStream_t)stream, a, (const T *)logits, labels, idx);
        DLKA_CHECK_LAUNCH();
        return DLKA_OK;
    });
}
