// Train-time augmentation of a batch of patches (include/dlka.h: dlka_augment_*): the apply half of get_moreDA_augmentation's train branch
// (3D/d_lka_former/training/data_augmentation/data_augmentation_moreDA.py:60-147), which the reference runs as batchgenerators transforms on
// scipy in four host processes.  Everything random is drawn by the caller (deformablelka_amd/augmentation.py: draw_*); every kernel here is a
// pure function of its inputs.
//
//   spatial   (a) SpatialTransform's interpolate_img for the image: a lane owns AUG_VPT output voxels that are neighbours along W, forms the
//             source coordinate of each in float64 from the voxel index and the sample's 3x4 map (the 3 x D x H x W coordinate grid the host
//             code builds is never stored), applies scipy.ndimage.map_coordinates' border rule, gathers 1 / 8 / 64 taps with scipy's weights
//             in scipy's order and stores in the input's type.  Order 3 reads float64 B-spline coefficients.  A sample flagged "plain" is a
//             copy of a box.
//   in-plane  (a) and (b) for the ACDC trainer's dummy-2D branch (Convert3DTo2DTransform around SpatialTransform, data_augmentation_moreDA.py:
//             54-75; batchgenerators' augment_spatial with dim == 2): arrays (B, P, H, W), every plane of a sample sampled at the same in-plane
//             coordinates from a 2x3 map.  The same kernels with RANK = 2: depth is no interpolation axis, so 1 / 4 / 16 taps, 4 neighbours
//             for the labels and coefficients filtered along H and W only.
//   labels    (b) the same coordinates for the label map.  Order 1 is batchgenerators' per-label rule (one map_coordinates of the indicator per
//             label, ascending, later labels overwrite where the result is >= 0.5) in ONE visit of the 8 neighbours: a label's interpolant is
//             the sum of the weights of the cells that hold it, so the per-label volumes are never written.
//   gaussian  (c) one axis of scipy.ndimage.gaussian_filter per launch: correlate1d's symmetric form, mode 'reflect', float64 sums, the
//             intermediate stored in the input's type between the axes as scipy stores it.
//   stats     (d) sum / sum of squares about the mean / min / max per (sample, channel) in float64: a lane walks its stride, a wave reduces by
//             shuffles, the workgroup folds its waves through LDS in wave order, a finish kernel folds the workgroups in index order.
//   pointwise (e) noise, brightness, contrast, gamma, the retain_stats map and the label replacement as a short list of steps per channel, one
//             streaming pass; the mirror is a reversed store index of that pass.
//
// No atomics: every output cell is computed by one lane, and the reductions have a fixed shape, so two runs give the same bits.
#include "cl_pipeline.h"

DLKA_LAUNCH_COUNTER(g_aug_launches, dlka_augment_launch_count)

namespace dlka {

#define AUG_THREADS 256
#define AUG_VPT 4                 // output voxels per lane along W
#define AUG_STAT_CHUNK 8192       // cells per workgroup of the statistics kernels (at least)
#define AUG_STAT_BLOCKS_MAX 256   // workgroups per channel (at most)
#define AUG_WROW (DLKA_AUG_RADIUS_MAX + 1)

// ---- storage types (loads: cl_pipeline.h) -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ void aug_st(float *p, long i, double v) { p[i] = (float)v; }
__device__ __forceinline__ void aug_st(double *p, long i, double v) { p[i] = v; }
__device__ __forceinline__ void aug_st(bf16_t *p, long i, double v) { p[i].v = bf16_bits((float)v); }   // through float, as torch converts
__device__ __forceinline__ void aug_st(int16_t *p, long i, double v)
{
    p[i] = v != v ? (int16_t)0 : (int16_t)(int)fmin(fmax(v, -32768.0), 32767.0);   // towards zero (numpy's astype), saturated
}
// what a store and a load of the storage type leave of a float64 value
template <typename T>
__device__ __forceinline__ double aug_round(double v)
{
    T t;
    aug_st(&t, 0, v);
    return ld_f64(&t, 0);
}

struct AugArgs {
    int B, C, order, mode, pad;
    int src[3], ext[3], out[3];      // ext: the coefficient array, src + 2 pad
    long src_cells, ext_cells, out_cells;
    double cval;
};

// What a lane knows about its AUG_VPT voxels.
struct AugLane {
    int b, c, oz, oy, ox0, nv;
};

__device__ __forceinline__ bool aug_lane(const AugArgs &a, int channels, AugLane &l)
{
    RowQuad q;
    if (!row_quad<AUG_VPT, AUG_THREADS>((long)a.B * channels * a.out[0] * a.out[1], a.out[2], q)) return false;
    long r = q.row;
    l.ox0 = q.x0;
    l.oy = (int)(r % a.out[1]);
    r /= a.out[1];
    l.oz = (int)(r % a.out[0]);
    r /= a.out[0];
    l.c = (int)(r % channels);
    l.b = (int)(r / channels);
    l.nv = q.nv;
    return true;
}

// The box of a plain sample, kept inside the source whatever the table says.  pl: (flag, lb of each of the RANK axes).
template <int RANK>
__device__ __forceinline__ long aug_plain_row(const AugArgs &a, const int *pl, const AugLane &l)
{
    const int y = min(max(l.oy + pl[RANK - 1], 0), a.src[1] - 1);
    if (RANK == 2) return (long)y * a.src[2];
    const int z = min(max(l.oz + pl[1], 0), a.src[0] - 1);
    return ((long)z * a.src[1] + y) * a.src[2];
}

// A tap beyond the array: scipy extends the coefficients by 'mirror' under 'constant' and by the edge cell under 'nearest'.
__device__ __forceinline__ int aug_tap(int i, int n, int mode)
{
    if (i >= 0 && i < n) return i;
    if (mode == DLKA_AUG_NEAREST || n == 1) return i < 0 ? 0 : n - 1;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

// One axis of one voxel: the coordinate in the array that is read (n cells), the first tap and the weights.  false: outside ('constant').
template <int ORDER>
__device__ __forceinline__ bool aug_axis(double cc, int n_src, int pad, int mode, int *idx, double *w)
{
#pragma clang fp contract(off)
    const int n = n_src + 2 * pad;
    if (!(cc == cc)) cc = -1.0;                                       // NaN: outside / the first cell
    if (mode == DLKA_AUG_CONSTANT) {
        if (cc < 0.0 || cc > (double)(n_src - 1)) return false;
    } else {
        cc = cc + (double)pad;
        cc = cc < 0.0 ? 0.0 : cc > (double)(n - 1) ? (double)(n - 1) : cc;
    }
    if (ORDER == 0) {
        idx[0] = aug_tap((int)floor(cc + 0.5), n, DLKA_AUG_NEAREST);
        w[0] = 1.0;
        return true;
    }
    const double f = floor(cc);
    const int lo = (int)f;
    const double y = cc - f;
    if (ORDER == 1) {
        idx[0] = aug_tap(lo, n, mode);
        idx[1] = aug_tap(lo + 1, n, mode);
        w[0] = 1.0 - y;
        w[1] = y;
        return true;
    }
    const double z = 1.0 - y;
    for (int k = 0; k < 4; ++k) idx[k] = aug_tap(lo - 1 + k, n, mode);
    w[1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
    w[2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0;
    w[0] = z * z * z / 6.0;
    w[3] = 1.0 - w[0] - w[1] - w[2];
    return true;
}

// cc[3 - RANK .. 2]: the source coordinate on the RANK interpolation axes from the sample's RANK x (RANK + 1) map.
template <int RANK>
__device__ __forceinline__ void aug_coordinate(const AugArgs &a, const double *m, int oz, int oy, int ox, double *cc)
{
#pragma clang fp contract(off)
    const double g1 = (double)oy - (double)(a.out[1] - 1) / 2.0, g2 = (double)ox - (double)(a.out[2] - 1) / 2.0;
    if (RANK == 2) {
        for (int d = 0; d < 2; ++d) cc[1 + d] = (m[3 * d] * g1 + m[3 * d + 1] * g2) + m[3 * d + 2];
        return;
    }
    const double g0 = (double)oz - (double)(a.out[0] - 1) / 2.0;
    for (int d = 0; d < 3; ++d) cc[d] = ((m[4 * d] * g0 + m[4 * d + 1] * g1) + m[4 * d + 2] * g2) + m[4 * d + 3];
}

// (a) ORDER 0 / 1: S = T, the image itself; ORDER 3: S = double, the coefficients.  RANK 2: the planes of a sample are its channels
// (a.C planes, a.src[0] = a.ext[0] = a.out[0] = 1), axis 0 has one tap at 0 and no weight.
template <typename T, typename S, int ORDER, int RANK>
__global__ void __launch_bounds__(AUG_THREADS) dlka_augment_spatial_kernel(AugArgs a, const T *x, const S *src, T *y, const double *maps,
                                                                              const int *plain)
{
#pragma clang fp contract(off)
    AugLane l;
    if (!aug_lane(a, a.C, l)) return;
    const long ch = (long)l.b * a.C + l.c;
    T *out = y + ((ch * a.out[0] + l.oz) * a.out[1] + l.oy) * a.out[2] + l.ox0;
    const int *pl = plain + (RANK + 1) * l.b;
    if (pl[0]) {
        const T *row = x + ch * a.src_cells + aug_plain_row<RANK>(a, pl, l);
        for (int v = 0; v < l.nv; ++v) out[v] = row[min(max(l.ox0 + v + pl[RANK], 0), a.src[2] - 1)];
        return;
    }
    constexpr int TAPS = ORDER == 3 ? 4 : ORDER + 1, TAPS0 = RANK == 3 ? TAPS : 1;
    const int pad = ORDER == 3 ? a.pad : 0;
    const int e1 = a.src[1] + 2 * pad, e2 = a.src[2] + 2 * pad;
    const S *p = src + ch * (ORDER == 3 ? a.ext_cells : a.src_cells);
    for (int v = 0; v < l.nv; ++v) {
        double cc[3], w[3][TAPS];
        int idx[3][TAPS];
        aug_coordinate<RANK>(a, maps + RANK * (RANK + 1) * l.b, l.oz, l.oy, l.ox0 + v, cc);
        bool inside = true;
        if (RANK == 2) idx[0][0] = 0;
        for (int d = 3 - RANK; d < 3; ++d) inside = aug_axis<ORDER>(cc[d], a.src[d], pad, a.mode, idx[d], w[d]) && inside;
        double t = a.cval;
        if (inside) {
            t = 0.0;
            for (int k0 = 0; k0 < TAPS0; ++k0)
                for (int k1 = 0; k1 < TAPS; ++k1) {
                    const S *row = p + ((long)idx[0][k0] * e1 + idx[1][k1]) * e2;
                    for (int k2 = 0; k2 < TAPS; ++k2) {
                        double coeff = ld_f64(row, idx[2][k2]);
                        if (ORDER > 0) {
                            if (RANK == 3) coeff = coeff * w[0][k0];
                            coeff = (coeff * w[1][k1]) * w[2][k2];
                        }
                        t = t + coeff;
                    }
                }
        }
        aug_st(out, v, t);
    }
}

// (b) RANK 2: the 4 in-plane neighbours.
template <int ORDER, int RANK>
__global__ void __launch_bounds__(AUG_THREADS) dlka_augment_labels_kernel(AugArgs a, const int *seg, int *y, const double *maps, const int *plain)
{
#pragma clang fp contract(off)
    AugLane l;
    if (!aug_lane(a, a.C, l)) return;
    const long ch = (long)l.b * a.C + l.c;
    int *out = y + ((ch * a.out[0] + l.oz) * a.out[1] + l.oy) * a.out[2] + l.ox0;
    const int *p = seg + ch * a.src_cells;
    const int *pl = plain + (RANK + 1) * l.b;
    if (pl[0]) {
        const int *row = p + aug_plain_row<RANK>(a, pl, l);
        for (int v = 0; v < l.nv; ++v) out[v] = row[min(max(l.ox0 + v + pl[RANK], 0), a.src[2] - 1)];
        return;
    }
    constexpr int TAPS = ORDER + 1, TAPS0 = RANK == 3 ? TAPS : 1;
    for (int v = 0; v < l.nv; ++v) {
        double cc[3], w[3][TAPS];
        int idx[3][TAPS];
        aug_coordinate<RANK>(a, maps + RANK * (RANK + 1) * l.b, l.oz, l.oy, l.ox0 + v, cc);
        bool inside = true;
        if (RANK == 2) {
            idx[0][0] = 0;
            w[0][0] = 1.0;
        }
        for (int d = 3 - RANK; d < 3; ++d) inside = aug_axis<ORDER>(cc[d], a.src[d], 0, a.mode, idx[d], w[d]) && inside;
        if (!inside) {                      // order 1: every label's interpolant is cval < 0.5
            out[v] = ORDER == 0 ? (int)a.cval : 0;
            continue;
        }
        if (ORDER == 0) {
            out[v] = p[((long)idx[0][0] * a.src[1] + idx[1][0]) * a.src[2] + idx[2][0]];
            continue;
        }
        int lab[8];
        double wt[8];
        int n = 0;
        for (int k0 = 0; k0 < TAPS0; ++k0)
            for (int k1 = 0; k1 < TAPS; ++k1)
                for (int k2 = 0; k2 < TAPS; ++k2) {
                    lab[n] = p[((long)idx[0][k0] * a.src[1] + idx[1][k1]) * a.src[2] + idx[2][k2]];
                    wt[n] = ((1.0 * w[0][k0]) * w[1][k1]) * w[2][k2];      // rank 2: w[0][0] is 1.0, which changes no bit
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
            if (s >= 0.5 && (!found || lab[k] > res)) {
                found = true;
                res = lab[k];
            }
        }
        out[v] = res;
    }
}

// (c)
__device__ __forceinline__ int aug_reflect(int i, int n)
{
    if (i >= 0 && i < n) return i;
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}

template <typename T>
__global__ void __launch_bounds__(AUG_THREADS) dlka_augment_gaussian_kernel(const T *x, T *y, long total, int e0, int e1, int e2, int axis,
                                                                               const int *radius, const double *weights)
{
#pragma clang fp contract(off)
    const long q = (long)blockIdx.x * AUG_THREADS + threadIdx.x;
    if (q >= total) return;
    const long cells = (long)e0 * e1 * e2;
    const long ch = q / cells, cell = q - ch * cells;
    const int r = radius[ch];
    if (r < 0) {
        y[q] = x[q];
        return;
    }
    const int i2 = (int)(cell % e2), i1 = (int)((cell / e2) % e1), i0 = (int)(cell / ((long)e2 * e1));
    const int n = axis == 0 ? e0 : axis == 1 ? e1 : e2, pos = axis == 0 ? i0 : axis == 1 ? i1 : i2;
    const long s = axis == 0 ? (long)e1 * e2 : axis == 1 ? (long)e2 : 1L;
    const T *line = x + q - (long)pos * s;
    const double *w = weights + ch * AUG_WROW;
    double tmp = ld_f64(line, (long)pos * s) * w[0];
    for (int j = r; j >= 1; --j)
        tmp = tmp + (ld_f64(line, (long)aug_reflect(pos - j, n) * s) + ld_f64(line, (long)aug_reflect(pos + j, n) * s)) * w[j];
    aug_st(y, q, tmp);
}

// (d) pass 0: sum, min, max; pass 1: the sum of squares about the mean of pass 0.  partials: [channel][workgroup][3].
template <typename T>
__global__ void __launch_bounds__(AUG_THREADS) dlka_augment_stats_kernel(const T *x, const double *stats, double *partials, long cells, int pass)
{
#pragma clang fp contract(off)
    __shared__ double sh[3][AUG_THREADS / 64];
    const int nblk = (int)gridDim.x, j = (int)blockIdx.x, ch = (int)blockIdx.y, tid = (int)threadIdx.x;
    const long chunk = cdivl(cells, nblk), lo = j * chunk, hi = lo + chunk < cells ? lo + chunk : cells;
    const T *p = x + (long)ch * cells;
    const double mean = pass ? stats[4 * ch] / (double)cells : 0.0;
    double s = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();
    for (long i = lo + tid; i < hi; i += AUG_THREADS) {
        const double v = ld_f64(p, i), d = v - mean;
        s = s + (pass ? d * d : v);
        mn = fmin(mn, v);
        mx = fmax(mx, v);
    }
    for (int off = 32; off >= 1; off >>= 1) {
        s = s + __shfl_down(s, off);
        mn = fmin(mn, __shfl_down(mn, off));
        mx = fmax(mx, __shfl_down(mx, off));
    }
    if ((tid & 63) == 0) {
        sh[0][tid >> 6] = s;
        sh[1][tid >> 6] = mn;
        sh[2][tid >> 6] = mx;
    }
    __syncthreads();
    if (tid == 0) {
        for (int wv = 1; wv < AUG_THREADS / 64; ++wv) {
            s = s + sh[0][wv];
            mn = fmin(mn, sh[1][wv]);
            mx = fmax(mx, sh[2][wv]);
        }
        double *o = partials + ((long)ch * nblk + j) * 3;
        o[0] = s;
        o[1] = mn;
        o[2] = mx;
    }
}

__global__ void __launch_bounds__(AUG_THREADS) dlka_augment_stats_finish_kernel(const double *partials, double *stats, int channels, int nblk,
                                                                                   int pass)
{
#pragma clang fp contract(off)
    const int ch = (int)(blockIdx.x * AUG_THREADS + threadIdx.x);
    if (ch >= channels) return;
    const double *p = partials + (long)ch * nblk * 3;
    double s = p[0], mn = p[1], mx = p[2];
    for (int j = 1; j < nblk; ++j) {
        s = s + p[3 * j];
        mn = fmin(mn, p[3 * j + 1]);
        mx = fmax(mx, p[3 * j + 2]);
    }
    if (pass) {
        stats[4 * ch + 1] = s;
    } else {
        stats[4 * ch] = s;
        stats[4 * ch + 2] = mn;
        stats[4 * ch + 3] = mx;
    }
}

// (e)
struct AugPw {
    int B, C, e0, e1, e2;
    long cells;
};

template <typename T>
__global__ void __launch_bounds__(AUG_THREADS) dlka_augment_pointwise_kernel(AugPw a, const T *x, const T *noise, T *y, const double *ops,
                                                                                const double *st0, const double *st1, const int *flip)
{
#pragma clang fp contract(off)
    RowQuad q;
    if (!row_quad<AUG_VPT, AUG_THREADS>((long)a.B * a.C * a.e0 * a.e1, a.e2, q)) return;
    long r = q.row;
    const int x0 = q.x0, nv = q.nv;
    const int iy = (int)(r % a.e1);
    r /= a.e1;
    const int iz = (int)(r % a.e0);
    const long ch = r / a.e0;
    const int fl = flip ? flip[ch / a.C] : 0;
    const long in = ch * a.cells + ((long)iz * a.e1 + iy) * a.e2 + x0;
    const long orow = ch * a.cells + ((long)((fl & 1) ? a.e0 - 1 - iz : iz) * a.e1 + ((fl & 2) ? a.e1 - 1 - iy : iy)) * a.e2;
    const double *op = ops + ch * (DLKA_AUG_OPS_MAX * 6);
    const double n_cells = (double)a.cells;
    for (int v = 0; v < nv; ++v) {
        double t = ld_f64(x, in + v);
        for (int k = 0; k < DLKA_AUG_OPS_MAX; ++k) {
            const double *o = op + 6 * k;
            const int code = (int)o[0];
            if (code == DLKA_AUG_OP_NONE) continue;
            if (code == DLKA_AUG_OP_NOISE) {
                t = t + ld_f64(noise, in + v);
            } else if (code == DLKA_AUG_OP_SCALE_ADD) {
                t = t * o[1] + o[2];
            } else if (code == DLKA_AUG_OP_CONTRAST) {
                const double *s = st0 + 4 * ch;
                const double mean = s[0] / n_cells;
                t = fmin(fmax((t - mean) * o[1] + mean, s[2]), s[3]);
            } else if (code == DLKA_AUG_OP_GAMMA) {
                const double *s = st0 + 4 * ch;
                const double sign = o[2], range = s[3] - s[2], mn = sign < 0.0 ? -s[3] : s[2];
                t = sign * (pow((sign * t - mn) / (range + 1e-7), o[1]) * range + mn);
            } else if (code == DLKA_AUG_OP_RETAIN) {
                const double *s = st0 + 4 * ch, *u = st1 + 4 * ch;
                t = (t - u[0] / n_cells) / (sqrt(u[1] / n_cells) + 1e-8) * sqrt(s[1] / n_cells) + s[0] / n_cells;
            } else if (code == DLKA_AUG_OP_REPLACE) {
                t = t == o[1] ? o[2] : t;
            }
            t = aug_round<T>(t);
        }
        const int ix = x0 + v;
        aug_st(y, orow + ((fl & 4) ? a.e2 - 1 - ix : ix), t);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
static long aug_blocks(long rows, int W) { return row_quad_blocks(rows, W, AUG_VPT, AUG_THREADS); }
static long aug_blocks(const AugArgs &a) { return aug_blocks((long)a.B * a.C * a.out[0] * a.out[1], a.out[2]); }

// rank 2: the description's src[0..1] / out[0..1] are (H, W) and its third entries are 0; the kernels see a depth of one cell that is never
// padded, and C planes per sample.
static int aug_check(const dlka_augment_desc *d, AugArgs *a, int rank)
{
    if (!d) return DLKA_ERR_NULL;
    if (d->B < 1 || d->C < 1 || d->pad < 0) return DLKA_ERR_SHAPE;
    if (d->mode != DLKA_AUG_CONSTANT && d->mode != DLKA_AUG_NEAREST) return DLKA_ERR_UNSUPPORTED;
    if (d->pad > 64) return DLKA_ERR_UNSUPPORTED;
    if (rank == 2 && (d->src[2] != 0 || d->out[2] != 0)) return DLKA_ERR_SHAPE;
    long sc = 1, ec = 1, oc = 1;
    a->src[0] = a->ext[0] = a->out[0] = 1;
    const int64_t pad[3] = {d->pad, d->pad, d->pad};
    const int o = 3 - rank;                   // the description's axes start at the kernels' axis o
    const int rc = check_extents(rank, {{d->src, 0x7fffffffL - 128, a->src + o, &sc, nullptr},
                                        {d->src, 0x7fffffffL - 128, a->ext + o, &ec, pad},
                                        {d->out, 0x7fffffffL, a->out + o, &oc, nullptr}});
    if (rc != DLKA_OK) return rc;
    a->B = d->B;
    a->C = d->C;
    a->order = d->order;
    a->mode = d->mode;
    a->pad = d->pad;
    a->src_cells = sc;
    a->ext_cells = ec;
    a->out_cells = oc;
    a->cval = d->cval;
    if (aug_blocks(*a) > 0x7fffffffL) return DLKA_ERR_UNSUPPORTED;
    return DLKA_OK;
}

template <int RANK>
static int aug_spatial(const void *x, const double *coef, void *y, const dlka_augment_desc *d, const double *maps, const int32_t *plain,
                       void *stream)
{
    AugArgs a;
    const int rc = aug_check(d, &a, RANK);
    if (rc != DLKA_OK) return rc;
    if (!x || !y || !maps || !plain) return DLKA_ERR_NULL;
    if (x == y) return DLKA_ERR_UNSUPPORTED;
    if (d->order != 0 && d->order != 1 && d->order != 3) return DLKA_ERR_UNSUPPORTED;
    if (d->order == 3 && !coef) return DLKA_ERR_NULL;
    if (d->order != 3 && d->pad != 0) return DLKA_ERR_UNSUPPORTED;
    return dispatch_storage<ST_ANY>(d->dtype, [&](auto t) -> int {
        using T = DLKA_T(t);
        g_aug_launches.add();
        const dim3 grid((unsigned)aug_blocks(a)), block(AUG_THREADS);
        hipStream_t st = (hipStream_t)stream;
        if (a.order == 0)
            DLKA_LAUNCH((dlka_augment_spatial_kernel<T, T, 0, RANK>), grid, block, 0, st, a, (const T *)x, (const T *)x, (T *)y, maps, plain);
        else if (a.order == 1)
            DLKA_LAUNCH((dlka_augment_spatial_kernel<T, T, 1, RANK>), grid, block, 0, st, a, (const T *)x, (const T *)x, (T *)y, maps, plain);
        else
            DLKA_LAUNCH((dlka_augment_spatial_kernel<T, double, 3, RANK>), grid, block, 0, st, a, (const T *)x, coef, (T *)y, maps, plain);
        DLKA_CHECK_LAUNCH();
        return DLKA_OK;
    });
}

template <int RANK>
static int aug_spatial_labels(const int32_t *seg, int32_t *out, const dlka_augment_desc *d, const double *maps, const int32_t *plain,
                              void *stream)
{
    AugArgs a;
    const int rc = aug_check(d, &a, RANK);
    if (rc != DLKA_OK) return rc;
    if (!seg || !out || !maps || !plain) return DLKA_ERR_NULL;
    if (seg == out || d->pad != 0) return DLKA_ERR_UNSUPPORTED;
    if (d->order != 0 && d->order != 1) return DLKA_ERR_UNSUPPORTED;
    if (d->order == 1 && d->mode == DLKA_AUG_CONSTANT && !(d->cval < 0.5)) return DLKA_ERR_UNSUPPORTED;
    if (d->order == 0 && !(d->cval >= -2147483648.0 && d->cval <= 2147483647.0)) return DLKA_ERR_UNSUPPORTED;
    g_aug_launches.add();
    const dim3 grid((unsigned)aug_blocks(a)), block(AUG_THREADS);
    if (d->order == 0)
        DLKA_LAUNCH((dlka_augment_labels_kernel<0, RANK>), grid, block, 0, (hipStream_t)stream, a, seg, out, maps, plain);
    else
        DLKA_LAUNCH((dlka_augment_labels_kernel<1, RANK>), grid, block, 0, (hipStream_t)stream, a, seg, out, maps, plain);
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}

}  // namespace dlka

using namespace dlka;

extern "C" int dlka_augment_spatial(const void *x, const double *coef, void *y, const dlka_augment_desc *d, const double *maps,
                                    const int32_t *plain, void *stream)
{
    return aug_spatial<3>(x, coef, y, d, maps, plain, stream);
}

extern "C" int dlka_augment_spatial_labels(const int32_t *seg, int32_t *out, const dlka_augment_desc *d, const double *maps,
                                           const int32_t *plain, void *stream)
{
    return aug_spatial_labels<3>(seg, out, d, maps, plain, stream);
}

extern "C" int dlka_augment_spatial2d(const void *x, const double *coef, void *y, const dlka_augment_desc *d, const double *maps,
                                      const int32_t *plain, void *stream)
{
    return aug_spatial<2>(x, coef, y, d, maps, plain, stream);
}

extern "C" int dlka_augment_spatial2d_labels(const int32_t *seg, int32_t *out, const dlka_augment_desc *d, const double *maps,
                                             const int32_t *plain, void *stream)
{
    return aug_spatial_labels<2>(seg, out, d, maps, plain, stream);
}

extern "C" int dlka_augment_gaussian(const void *x, void *y, int dtype, int64_t channels, const int64_t *ext, int axis, const int32_t *radius,
                                     const double *weights, void *stream)
{
    if (!x || !y || !ext || !radius || !weights) return DLKA_ERR_NULL;
    if (x == y) return DLKA_ERR_UNSUPPORTED;
    if (axis < 0 || axis > 2 || channels < 1) return DLKA_ERR_SHAPE;
    return dispatch_storage<ST_ANY>(dtype, [&](auto t) -> int {
        using T = DLKA_T(t);
        long cells = 1;
        int e[3];
        const int rc = check_extents(3, {{ext, 0x3fffffffL, e, &cells, nullptr}});
        if (rc != DLKA_OK) return rc;
        if (channels > 0x7fffffffL || cells * channels > 0x7fffffffL * (long)AUG_THREADS) return DLKA_ERR_UNSUPPORTED;
        const long total = cells * channels;
        g_aug_launches.add();
        DLKA_LAUNCH(dlka_augment_gaussian_kernel<T>, dim3((unsigned)cdivl(total, AUG_THREADS)), dim3(AUG_THREADS), 0, (hipStream_t)stream,
                    (const T *)x, (T *)y, total, e[0], e[1], e[2], axis, radius, weights);
        DLKA_CHECK_LAUNCH();
        return DLKA_OK;
    });
}

static int aug_stat_blocks(long cells)
{
    const long n = cdivl(cells, AUG_STAT_CHUNK);
    return (int)(n < 1 ? 1 : n > AUG_STAT_BLOCKS_MAX ? AUG_STAT_BLOCKS_MAX : n);
}

extern "C" size_t dlka_augment_stats_workspace_bytes(int64_t channels, int64_t cells)
{
    if (channels < 1 || cells < 1) return 0;
    return (size_t)channels * (size_t)aug_stat_blocks(cells) * 3 * sizeof(double);
}

extern "C" int dlka_augment_channel_stats(const void *x, double *stats, void *workspace, size_t workspace_bytes, int dtype, int64_t channels,
                                          int64_t cells, void *stream)
{
    if (!x || !stats) return DLKA_ERR_NULL;
    if (channels < 1 || cells < 1) return DLKA_ERR_SHAPE;
    if (channels > 65535 || cells > 0x7fffffffL) return DLKA_ERR_UNSUPPORTED;
    return dispatch_storage<ST_ANY>(dtype, [&](auto t) -> int {
        using T = DLKA_T(t);
        if (!workspace || workspace_bytes < dlka_augment_stats_workspace_bytes(channels, cells)) return DLKA_ERR_WORKSPACE;
        if (((uintptr_t)workspace & 7) != 0) return DLKA_ERR_WORKSPACE;
        g_aug_launches.add(4);
        hipStream_t st = (hipStream_t)stream;
        double *partials = (double *)workspace;
        const int nblk = aug_stat_blocks(cells);
        for (int pass = 0; pass < 2; ++pass) {
            DLKA_LAUNCH(dlka_augment_stats_kernel<T>, dim3((unsigned)nblk, (unsigned)channels), dim3(AUG_THREADS), 0, st, (const T *)x,
                        (const double *)stats, partials, (long)cells, pass);
            DLKA_LAUNCH(dlka_augment_stats_finish_kernel, dim3((unsigned)cdivl(channels, AUG_THREADS)), dim3(AUG_THREADS), 0, st,
                        (const double *)partials, stats, (int)channels, nblk, pass);
        }
        DLKA_CHECK_LAUNCH();
        return DLKA_OK;
    });
}

extern "C" int dlka_augment_pointwise(const void *x, const void *noise, void *y, int dtype, int64_t B, int64_t C, const int64_t *ext,
                                      const double *ops, const double *stats0, const double *stats1, const int32_t *flip, void *stream)
{
    if (!x || !y || !ext || !ops) return DLKA_ERR_NULL;
    if (x == y) return DLKA_ERR_UNSUPPORTED;
    if (B < 1 || C < 1) return DLKA_ERR_SHAPE;
    return dispatch_storage<ST_ANY>(dtype, [&](auto t) -> int {
        using T = DLKA_T(t);
        AugPw a;
        int e[3];
        a.cells = 1;
        const int rc = check_extents(3, {{ext, 0x7fffffffL, e, &a.cells, nullptr}});
        if (rc != DLKA_OK) return rc;
        if (B > 0x7fffffffL || C > 0x7fffffffL || B * C > 0x7fffffffL) return DLKA_ERR_UNSUPPORTED;
        a.B = (int)B;
        a.C = (int)C;
        a.e0 = e[0];
        a.e1 = e[1];
        a.e2 = e[2];
        const long blocks = aug_blocks(B * C * a.e0 * a.e1, a.e2);
        if (blocks > 0x7fffffffL) return DLKA_ERR_UNSUPPORTED;
        g_aug_launches.add();
        DLKA_LAUNCH(dlka_augment_pointwise_kernel<T>, dim3((unsigned)blocks), dim3(AUG_THREADS), 0, (hipStream_t)stream, a, (const T *)x,
                    (const T *)noise, (T *)y, ops, stats0, stats1, flip);
        DLKA_CHECK_LAUNCH();
        return DLKA_OK;
    });
}
