// Cubic B-spline coefficients of a volume (include/dlka.h: dlka_spline_*): what scipy.ndimage.spline_filter computes in front of every order-3
// interpolation, for the resampling (cl_resample.hip), the train-time augmentation (cl_augment.hip) and the 2-D evaluator (cl_zoom2d.hip),
// whose evaluation kernels read the coefficients.  float64 throughout.
//
//   pad        edge samples on both sides of every axis and the cast to float64 in one pass (pad 0: the cast alone).
//   prefilter  in place along one axis: gain, causal pass from the boundary's start value, anti-causal pass.  One lane per line.  The two
//              boundaries are scipy's: 'reflect' (d c b a | a b c d | d c b a; its 'nearest' is this one on the padded array) and 'mirror'
//              (d c b | a b c d | c b a; what it uses under 'constant').  They differ in the period of the start value's sum and in the
//              initialisation of the last cell; the rest is written once.
//
// No atomics, no reduction across lanes: two runs give the same bits.
#include "cl_resample.h"

namespace dlka {

#define SPL_THREADS 256
#define SPL_PAD_MAX 64

struct SplPad {
    int in[3], pad[3], ext[3];
    long cells;
};

template <typename T>
__global__ void __launch_bounds__(SPL_THREADS) dlka_spline_pad_kernel(SplPad a, const T *x, double *p)
{
    const long q = (long)blockIdx.x * SPL_THREADS + threadIdx.x;
    if (q >= a.cells) return;
    const int pw = (int)(q % a.ext[2]);
    const int ph = (int)((q / a.ext[2]) % a.ext[1]);
    const int pd = (int)(q / ((long)a.ext[2] * a.ext[1]));
    const int sw = min(max(pw - a.pad[2], 0), a.in[2] - 1);
    const int sh = min(max(ph - a.pad[1], 0), a.in[1] - 1);
    const int sd = min(max(pd - a.pad[0], 0), a.in[0] - 1);
    p[q] = (double)x[((long)sd * a.in[1] + sh) * a.in[2] + sw];
}

// scipy.ndimage.spline_filter1d(order=3) of every line along `axis`.  Contraction is off and the operations keep scipy's order, per boundary.
template <int BOUNDARY>
__global__ void __launch_bounds__(SPL_THREADS) dlka_spline_prefilter_kernel(double *p, int e0, int e1, int e2, int axis)
{
#pragma clang fp contract(off)
    const int ext[3] = {e0, e1, e2};
    const long stride[3] = {(long)e1 * e2, (long)e2, 1L};
    const int n = ext[axis];
    const int ua = axis == 0 ? 1 : 0, ub = axis == 2 ? 1 : 2;   // the two other axes
    const long lines = (long)ext[ua] * ext[ub];
    const long q = (long)blockIdx.x * SPL_THREADS + threadIdx.x;
    if (q >= lines || n < 2) return;
    double *c = p + (q / ext[ub]) * stride[ua] + (q % ext[ub]) * stride[ub];
    const long s = stride[axis];
    const double z = -0.26794919243112270647;   // sqrt(3) - 2
    const double gain = (1.0 - z) * (1.0 - 1.0 / z);
    for (int i = 0; i < n; ++i) c[i * s] *= gain;
    // the causal start value: the sum over one period of the extended line, 2 n cells ('reflect') or 2 n - 2 ('mirror'), folded in half
    const int m = BOUNDARY == DLKA_SPLINE_MIRROR ? n - 1 : n;
    double z_m = 1.0;
    for (int i = 0; i < m; ++i) z_m *= z;
    double z_i = z;
    const double c0 = c[0];
    double acc = c0 + z_m * c[(long)(n - 1) * s];
    for (int i = 1; i < m; ++i) {
        acc += z_i * (c[i * s] + z_m * c[(long)(n - 1 - i) * s]);
        z_i *= z;
    }
    if (BOUNDARY == DLKA_SPLINE_MIRROR) {
        c[0] = acc / (1.0 - z_m * z_m);
    } else {
        acc *= z / (1.0 - z_m * z_m);
        c[0] = acc + c0;
    }
    for (int i = 1; i < n; ++i) c[i * s] += z * c[(long)(i - 1) * s];
    if (BOUNDARY == DLKA_SPLINE_MIRROR)
        c[(long)(n - 1) * s] = (z * c[(long)(n - 2) * s] + c[(long)(n - 1) * s]) * z / (z * z - 1.0);
    else
        c[(long)(n - 1) * s] *= z / (z - 1.0);
    for (int i = n - 2; i >= 0; --i) c[i * s] = z * (c[(long)(i + 1) * s] - c[i * s]);
}

}  // namespace dlka

using namespace dlka;

extern "C" int dlka_spline_pad(const void *x, double *padded, int dtype, const int64_t *in, const int64_t *pad, void *stream)
{
    if (!x || !padded || !in || !pad) return DLKA_ERR_NULL;
    return dispatch_storage<ST_F32 | ST_F64>(dtype, [&](auto t) -> int {
        using T = DLKA_T(t);
        SplPad a;
        a.cells = 1;
        const int rc = check_extents(3, {{in, 0x7fffffffL - 2 * SPL_PAD_MAX, a.ext, &a.cells, pad}}, [&](int ax) {
            return pad[ax] < 0 ? (int)DLKA_ERR_SHAPE : pad[ax] > SPL_PAD_MAX ? (int)DLKA_ERR_UNSUPPORTED : (int)DLKA_OK;
        });
        if (rc != DLKA_OK) return rc;
        for (int ax = 0; ax < 3; ++ax) {
            a.in[ax] = (int)in[ax];
            a.pad[ax] = (int)pad[ax];
        }
        g_rs_launches.add();
        DLKA_LAUNCH(dlka_spline_pad_kernel<T>, dim3((unsigned)cdivl(a.cells, SPL_THREADS)), dim3(SPL_THREADS), 0, (hipStream_t)stream, a,
                    (const T *)x, padded);
        DLKA_CHECK_LAUNCH();
        return DLKA_OK;
    });
}

extern "C" int dlka_spline_prefilter(double *coef, const int64_t *ext, int axis, int boundary, void *stream)
{
    if (!coef || !ext) return DLKA_ERR_NULL;
    if (axis < 0 || axis > 2) return DLKA_ERR_SHAPE;
    if (boundary != DLKA_SPLINE_REFLECT && boundary != DLKA_SPLINE_MIRROR) return DLKA_ERR_UNSUPPORTED;
    long cells = 1;
    int e[3];
    const int rc = check_extents(3, {{ext, 0x7fffffffL, e, &cells, nullptr}});
    if (rc != DLKA_OK) return rc;
    g_rs_launches.add();
    dispatch_menu<DLKA_SPLINE_MIRROR, DLKA_SPLINE_REFLECT>(boundary, [&](auto b) {
        DLKA_LAUNCH(dlka_spline_prefilter_kernel<DLKA_V(b)>, dim3((unsigned)cdivl(cells / e[axis], SPL_THREADS)), dim3(SPL_THREADS), 0,
                    (hipStream_t)stream, coef, e[0], e[1], e[2], axis);
    });
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}
