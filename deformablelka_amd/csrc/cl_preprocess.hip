// nnU-Net's case preprocessing (include/dlka.h: dlka_prep_*): what ImageCropper.crop (3D/d_lka_former/preprocessing/cropping.py:23-150) and
// the normalisation loop of GenericPreprocessor.resample_and_normalize (preprocessing/preprocessing.py:274-305) compute on one host core with
// scipy.ndimage.binary_fill_holes, two full-volume copies and one numpy pass per modality.
//
//   background  (a) 1 where every channel of a cell is == 0 (a NaN is != 0).  The caller labels this map with dlka_cc_components, connectivity 1.
//   faces       (b) one visit of the cells on the 2 * rank faces of the component map: flag[component] = 1, the same byte from every writer.
//   fill        (c) mask = !background | !flag[component]: a background component that touches no face is a hole (binary_fill_holes: the
//               complement of what a dilation of the border reaches inside the background).  In the same visit the minimum and maximum index
//               per axis and the count of the set cells: lanes, then the wave (__shfl_down), then the workgroup (LDS), then six integer
//               atomicMin / atomicMax and one integer atomicAdd per workgroup.
//   crop        (d) the box of every channel, NaN -> 0 on request, and the label map with nonzero_label outside the mask.
//   stats       (e) per channel count, mean and population standard deviation of the selected cells in float64, two passes (the mean, then the
//               squared deviations about it): a lane walks its stride, a wave reduces by __shfl_down, the workgroup's waves and then the
//               workgroups are added in index order.  The same fixed order as the channel statistics of cl_augment.hip, which fold
//               (sum, min, max) triples over every cell and therefore keep their own kernels.
//   normalize   (f) one launch for all channels; the scheme, bounds, mean and sd of a channel come from its record in a device table that (e)
//               completes, so nothing is read back between the statistics and the apply.
//
// All of them stream: a lane owns PREP_PER consecutive cells of the contiguous axis and moves them with one 16-byte access per array when the
// addresses allow it (float and int32 arrays; 4 bytes of a uint8 map), cell by cell otherwise and in the tail.
//
// Determinism: minima, maxima and integer sums do not depend on the order the atomics land in; the float64 sums are folded in a fixed order
// without atomics.  Two runs give the same bits in every output.
#include "cl_pipeline.h"

DLKA_LAUNCH_COUNTER(g_prep_launches, dlka_prep_launch_count)

namespace dlka {

#define PREP_THREADS 256
#define PREP_PER 4
#define PREP_WAVES (PREP_THREADS / 64)
#define PREP_STAT_CHUNK 16384L            // cells per workgroup of the statistics until PREP_STAT_BLOCKS_MAX workgroups per channel are in use
#define PREP_STAT_BLOCKS_MAX 1024
#define PREP_INT_MAX 0x7fffffff

typedef int i32x4 __attribute__((ext_vector_type(4)));

struct PrepArgs {
    int rank, C, S, nan0, label, has_seg;
    int ext[3], lo[3], cext[3];
    long N, NC;                           // cells of the volume, cells of the box
};

__device__ __forceinline__ bool prep_aligned(const void *p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ void prep_atomic_min(int *p, int v)
{
#if defined(HIPEMU)
    __atomic_fetch_min(p, v, __ATOMIC_RELAXED);
#else
    atomicMin(p, v);
#endif
}
__device__ __forceinline__ void prep_atomic_max(int *p, int v)
{
#if defined(HIPEMU)
    __atomic_fetch_max(p, v, __ATOMIC_RELAXED);
#else
    atomicMax(p, v);
#endif
}

// (a)
__global__ __launch_bounds__(PREP_THREADS) void dlka_prep_background_kernel(const float *__restrict__ x, unsigned char *__restrict__ bg, long N, int C)
{
    const long i0 = ((long)blockIdx.x * PREP_THREADS + threadIdx.x) * PREP_PER;
    if (i0 >= N) return;
    const bool vec = i0 + PREP_PER <= N && prep_aligned(x) && (C == 1 || (N & 3) == 0) && prep_aligned(bg);
    if (vec) {
        bool z0 = true, z1 = true, z2 = true, z3 = true;
        for (int c = 0; c < C; ++c) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(x + c * N + i0);
            z0 = z0 && !(v[0] != 0.f); z1 = z1 && !(v[1] != 0.f); z2 = z2 && !(v[2] != 0.f); z3 = z3 && !(v[3] != 0.f);
        }
        *reinterpret_cast<unsigned *>(bg + i0) = (z0 ? 1u : 0u) | (z1 ? 0x100u : 0u) | (z2 ? 0x10000u : 0u) | (z3 ? 0x1000000u : 0u);
        return;
    }
    const int n = N - i0 < PREP_PER ? (int)(N - i0) : PREP_PER;
    for (int k = 0; k < n; ++k) {
        bool z = true;
        for (int c = 0; c < C; ++c) z = z && !(x[c * N + i0 + k] != 0.f);
        bg[i0 + k] = z ? 1 : 0;
    }
}

// box[8] = minima (3), maxima (3), count, unused
__global__ void dlka_prep_box_init_kernel(int *__restrict__ box)
{
    const int t = (int)threadIdx.x;
    if (t < 8) box[t] = t < 3 ? PREP_INT_MAX : t < 6 ? -1 : 0;
}

// (b) blockIdx.y = 2 * (axis - (3 - rank)) + side; blockIdx.x walks the plane of the two other axes
__global__ __launch_bounds__(PREP_THREADS) void dlka_prep_faces_kernel(const int *__restrict__ labels, unsigned char *__restrict__ flag, const PrepArgs a)
{
    const int f = (int)blockIdx.y, ax = 3 - a.rank + (f >> 1), side = f & 1;
    const int u = ax == 0 ? 1 : 0, v = ax == 2 ? 1 : 2;
    const long plane = (long)a.ext[u] * a.ext[v];
    const long p = (long)blockIdx.x * PREP_THREADS + threadIdx.x;
    if (p >= plane) return;
    int idx[3];
    idx[ax] = side ? a.ext[ax] - 1 : 0;   // (an axis of extent 1: both sides are its only plane, and every cell lies on it)
    idx[u] = (int)(p / a.ext[v]);
    idx[v] = (int)(p - (long)idx[u] * a.ext[v]);
    const long lab = labels[((long)idx[0] * a.ext[1] + idx[1]) * a.ext[2] + idx[2]];
    if (lab > 0 && lab <= a.N) flag[lab] = 1;
}

// (c) labels != NULL: in = the background map, set = !in | !flag[label]; labels == NULL: set = in != 0 (the box of a given mask).  mask may be NULL.
__global__ __launch_bounds__(PREP_THREADS) void dlka_prep_fill_kernel(const unsigned char *__restrict__ in, const int *__restrict__ labels,
                                                                      const unsigned char *__restrict__ flag, unsigned char *__restrict__ mask,
                                                                      int *__restrict__ box, const PrepArgs a)
{
    __shared__ int sh[7][PREP_WAVES];
    const int tid = (int)threadIdx.x;
    const long i0 = ((long)blockIdx.x * PREP_THREADS + tid) * PREP_PER;
    int r[7] = {PREP_INT_MAX, PREP_INT_MAX, PREP_INT_MAX, -1, -1, -1, 0};
    if (i0 < a.N) {
        const int n = a.N - i0 < PREP_PER ? (int)(a.N - i0) : PREP_PER;
        const bool vec = n == PREP_PER && prep_aligned(in) && prep_aligned(labels) && prep_aligned(mask);
        unsigned char b[PREP_PER] = {0, 0, 0, 0};
        int l[PREP_PER] = {0, 0, 0, 0};
        if (vec) {
            const unsigned w = *reinterpret_cast<const unsigned *>(in + i0);
            b[0] = (unsigned char)w; b[1] = (unsigned char)(w >> 8); b[2] = (unsigned char)(w >> 16); b[3] = (unsigned char)(w >> 24);
            if (labels) {
                const i32x4 q = *reinterpret_cast<const i32x4 *>(labels + i0);
                l[0] = q[0]; l[1] = q[1]; l[2] = q[2]; l[3] = q[3];
            }
        } else {
            for (int k = 0; k < n; ++k) {
                b[k] = in[i0 + k];
                if (labels) l[k] = labels[i0 + k];
            }
        }
        const long hw = (long)a.ext[1] * a.ext[2];
        int d = (int)(i0 / hw);
        const long rest = i0 - d * hw;
        int h = (int)(rest / a.ext[2]), w = (int)(rest - (long)h * a.ext[2]);
        unsigned packed = 0;
        for (int k = 0; k < n; ++k) {
            bool m;
            if (labels) m = !b[k] || !(l[k] > 0 && l[k] <= a.N && flag[l[k]]);
            else m = b[k] != 0;
            if (m) {
                packed |= 1u << (8 * k);
                r[0] = d < r[0] ? d : r[0]; r[1] = h < r[1] ? h : r[1]; r[2] = w < r[2] ? w : r[2];
                r[3] = d > r[3] ? d : r[3]; r[4] = h > r[4] ? h : r[4]; r[5] = w > r[5] ? w : r[5];
                r[6] += 1;
            }
            if (++w == a.ext[2]) { w = 0; if (++h == a.ext[1]) { h = 0; ++d; } }
        }
        if (mask) {
            if (vec) *reinterpret_cast<unsigned *>(mask + i0) = packed;
            else
                for (int k = 0; k < n; ++k) mask[i0 + k] = (unsigned char)((packed >> (8 * k)) & 1u);
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {     // (every lane of the workgroup arrives here)
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            const int o = __shfl_down(r[q], off);
            r[q] = q < 3 ? (o < r[q] ? o : r[q]) : q < 6 ? (o > r[q] ? o : r[q]) : r[q] + o;
        }
    }
    if ((tid & 63) == 0)
        for (int q = 0; q < 7; ++q) sh[q][tid >> 6] = r[q];
    __syncthreads();
    if (tid == 0) {
        for (int wv = 1; wv < PREP_WAVES; ++wv)
            for (int q = 0; q < 7; ++q) {
                const int o = sh[q][wv];
                r[q] = q < 3 ? (o < r[q] ? o : r[q]) : q < 6 ? (o > r[q] ? o : r[q]) : r[q] + o;
            }
        if (r[6] > 0) {
            for (int q = 0; q < 3; ++q) prep_atomic_min(box + q, r[q]);
            for (int q = 3; q < 6; ++q) prep_atomic_max(box + q, r[q]);
            atomicAdd(box + 6, r[6]);
        }
    }
}

// (d) a lane owns PREP_PER consecutive cells of the box
__global__ __launch_bounds__(PREP_THREADS) void dlka_prep_crop_kernel(const float *__restrict__ x, const int *__restrict__ seg,
                                                                      const unsigned char *__restrict__ mask, float *__restrict__ y,
                                                                      int *__restrict__ seg_out, const PrepArgs a)
{
    const long s0 = ((long)blockIdx.x * PREP_THREADS + threadIdx.x) * PREP_PER;
    if (s0 >= a.NC) return;
    const int n = a.NC - s0 < PREP_PER ? (int)(a.NC - s0) : PREP_PER;
    const long chw = (long)a.cext[1] * a.cext[2];
    int d = (int)(s0 / chw);
    const long rest = s0 - d * chw;
    int h = (int)(rest / a.cext[2]), w = (int)(rest - (long)h * a.cext[2]);
    long src[PREP_PER] = {0, 0, 0, 0};
    for (int k = 0; k < n; ++k) {
        src[k] = ((long)(d + a.lo[0]) * a.ext[1] + (h + a.lo[1])) * a.ext[2] + (w + a.lo[2]);
        if (++w == a.cext[2]) { w = 0; if (++h == a.cext[1]) { h = 0; ++d; } }
    }
    for (int c = 0; c < a.C; ++c) {
        float v[PREP_PER] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < n; ++k) {
            const float t = x[c * a.N + src[k]];
            v[k] = (a.nan0 && t != t) ? 0.f : t;
        }
        float *o = y + c * a.NC + s0;
        if (n == PREP_PER && prep_aligned(o)) *reinterpret_cast<f32x4 *>(o) = f32x4{v[0], v[1], v[2], v[3]};
        else
            for (int k = 0; k < n; ++k) o[k] = v[k];
    }
    if (!seg_out) return;
    unsigned char m[PREP_PER] = {0, 0, 0, 0};
    for (int k = 0; k < n; ++k) m[k] = mask[src[k]];
    for (int c = 0; c < a.S; ++c) {
        int v[PREP_PER] = {0, 0, 0, 0};
        for (int k = 0; k < n; ++k) {
            if (a.has_seg) {
                const int t = seg[c * a.N + src[k]];
                v[k] = (t == 0 && m[k] == 0) ? a.label : t;
            } else {
                v[k] = m[k] == 0 ? a.label : 0;
            }
        }
        int *o = seg_out + c * a.NC + s0;
        if (n == PREP_PER && prep_aligned(o)) *reinterpret_cast<i32x4 *>(o) = i32x4{v[0], v[1], v[2], v[3]};
        else
            for (int k = 0; k < n; ++k) o[k] = v[k];
    }
}

// table[channel][DLKA_PREP_REC] float64 = scheme, lower, upper, mean, sd, use_mask, count, unused
#define PREP_R_SCHEME 0
#define PREP_R_LOWER 1
#define PREP_R_UPPER 2
#define PREP_R_MEAN 3
#define PREP_R_SD 4
#define PREP_R_USE_MASK 5
#define PREP_R_COUNT 6

// selection of a channel's statistics: 0 every cell, 1 seg >= 0, 2 lower < x < upper
__device__ __forceinline__ int prep_selection(const double *rec)
{
    return (int)rec[PREP_R_SCHEME] == DLKA_PREP_CT2 ? 2 : (rec[PREP_R_USE_MASK] != 0.0 ? 1 : 0);
}

// (e) pass 0: sum and count; pass 1: the sum of squares about the mean of pass 0.  partials: [channel][workgroup][2].  A CT channel brings its
// statistics in the table: its workgroups have nothing to do.
__global__ __launch_bounds__(PREP_THREADS) void dlka_prep_stats_kernel(const float *__restrict__ x, const int *__restrict__ seg,
                                                                       const double *__restrict__ table, double *__restrict__ partials, long N,
                                                                       int pass)
{
#pragma clang fp contract(off)
    __shared__ double sh[2][PREP_WAVES];
    const int nblk = (int)gridDim.x, j = (int)blockIdx.x, ch = (int)blockIdx.y, tid = (int)threadIdx.x;
    const double *rec = table + (long)ch * DLKA_PREP_REC;
    if ((int)rec[PREP_R_SCHEME] == DLKA_PREP_CT) return;
    const int sel = prep_selection(rec);
    const float lower = (float)rec[PREP_R_LOWER], upper = (float)rec[PREP_R_UPPER];
    const double mean = pass ? rec[PREP_R_MEAN] : 0.0;
    const long chunk = cdivl(cdivl(N, nblk), PREP_PER) * PREP_PER, lo = j * chunk, hi = lo + chunk < N ? lo + chunk : N;
    const float *p = x + (long)ch * N;
    const bool al = prep_aligned(p) && (sel != 1 || prep_aligned(seg));
    double s = 0.0, cnt = 0.0;
    for (long i = lo + (long)tid * PREP_PER; i < hi; i += (long)PREP_THREADS * PREP_PER) {
        const int n = hi - i < PREP_PER ? (int)(hi - i) : PREP_PER;
        float v[PREP_PER] = {0.f, 0.f, 0.f, 0.f};
        int g[PREP_PER] = {0, 0, 0, 0};
        if (n == PREP_PER && al) {
            const f32x4 q = *reinterpret_cast<const f32x4 *>(p + i);
            v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
            if (sel == 1) {
                const i32x4 t = *reinterpret_cast<const i32x4 *>(seg + i);
                g[0] = t[0]; g[1] = t[1]; g[2] = t[2]; g[3] = t[3];
            }
        } else {
            for (int k = 0; k < n; ++k) {
                v[k] = p[i + k];
                if (sel == 1) g[k] = seg[i + k];
            }
        }
        for (int k = 0; k < n; ++k) {
            const bool take = sel == 0 ? true : sel == 1 ? g[k] >= 0 : (v[k] > lower && v[k] < upper);
            if (!take) continue;
            const double dv = (double)v[k] - mean;
            s = s + (pass ? dv * dv : dv);
            cnt = cnt + 1.0;
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        s = s + __shfl_down(s, off);
        cnt = cnt + __shfl_down(cnt, off);
    }
    if ((tid & 63) == 0) {
        sh[0][tid >> 6] = s;
        sh[1][tid >> 6] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        for (int wv = 1; wv < PREP_WAVES; ++wv) {
            s = s + sh[0][wv];
            cnt = cnt + sh[1][wv];
        }
        double *o = partials + ((long)ch * nblk + j) * 2;
        o[0] = s;
        o[1] = cnt;
    }
}

__global__ __launch_bounds__(PREP_THREADS) void dlka_prep_stats_finish_kernel(const double *__restrict__ partials, double *__restrict__ table,
                                                                              int channels, int nblk, int pass)
{
#pragma clang fp contract(off)
    const int ch = (int)(blockIdx.x * PREP_THREADS + threadIdx.x);
    if (ch >= channels) return;
    double *rec = table + (long)ch * DLKA_PREP_REC;
    if ((int)rec[PREP_R_SCHEME] == DLKA_PREP_CT) return;
    const double *p = partials + (long)ch * nblk * 2;
    double s = p[0], cnt = p[1];
    for (int j = 1; j < nblk; ++j) {
        s = s + p[2 * j];
        cnt = cnt + p[2 * j + 1];
    }
    if (pass) {
        rec[PREP_R_SD] = sqrt(s / cnt);
    } else {
        rec[PREP_R_MEAN] = s / cnt;
        rec[PREP_R_COUNT] = cnt;
    }
}

// preprocessing.py:276-305 for one cell, every step rounded to float32
__device__ __forceinline__ float prep_normalize_cell(float v, int g, int scheme, bool use_mask, float lower, float upper, float mean, float div)
{
#pragma clang fp contract(off)
    if (scheme == DLKA_PREP_NONCT) {
        if (use_mask && g < 0) return 0.f;
        return (v - mean) / div;
    }
    v = v < lower ? lower : v;            // (numpy.clip: a NaN stays a NaN)
    v = v > upper ? upper : v;
    v = (v - mean) / div;
    return (use_mask && g < 0) ? 0.f : v;
}

// (f) blockIdx.y = channel
__global__ __launch_bounds__(PREP_THREADS) void dlka_prep_normalize_kernel(const float *__restrict__ x, const int *__restrict__ seg,
                                                                           const double *__restrict__ table, float *__restrict__ y, long N)
{
#pragma clang fp contract(off)
    const int ch = (int)blockIdx.y;
    const long i0 = ((long)blockIdx.x * PREP_THREADS + threadIdx.x) * PREP_PER;
    if (i0 >= N) return;
    const double *rec = table + (long)ch * DLKA_PREP_REC;
    const int scheme = (int)rec[PREP_R_SCHEME];
    const bool use_mask = rec[PREP_R_USE_MASK] != 0.0;
    const float lower = (float)rec[PREP_R_LOWER], upper = (float)rec[PREP_R_UPPER], mean = (float)rec[PREP_R_MEAN];
    const float sd = (float)rec[PREP_R_SD];
    const float div = scheme == DLKA_PREP_NONCT ? sd + 1e-8f : sd;
    const float *p = x + (long)ch * N;
    float *o = y + (long)ch * N;
    const int n = N - i0 < PREP_PER ? (int)(N - i0) : PREP_PER;
    if (n == PREP_PER && prep_aligned(p) && prep_aligned(o) && (!use_mask || prep_aligned(seg))) {
        const f32x4 q = *reinterpret_cast<const f32x4 *>(p + i0);
        i32x4 g = {0, 0, 0, 0};
        if (use_mask) g = *reinterpret_cast<const i32x4 *>(seg + i0);
        f32x4 r;
        r[0] = prep_normalize_cell(q[0], g[0], scheme, use_mask, lower, upper, mean, div);
        r[1] = prep_normalize_cell(q[1], g[1], scheme, use_mask, lower, upper, mean, div);
        r[2] = prep_normalize_cell(q[2], g[2], scheme, use_mask, lower, upper, mean, div);
        r[3] = prep_normalize_cell(q[3], g[3], scheme, use_mask, lower, upper, mean, div);
        *reinterpret_cast<f32x4 *>(o + i0) = r;
        return;
    }
    for (int k = 0; k < n; ++k)
        o[i0 + k] = prep_normalize_cell(p[i0 + k], use_mask ? seg[i0 + k] : 0, scheme, use_mask, lower, upper, mean, div);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
static int prep_check(const dlka_prep_desc *d)
{
    if (!d) return DLKA_ERR_NULL;
    if (d->rank < 2 || d->rank > 3) return DLKA_ERR_SHAPE;
    if (d->C < 1) return DLKA_ERR_SHAPE;
    if (d->C > DLKA_PREP_C_MAX) return DLKA_ERR_UNSUPPORTED;
    long cells = 1;                           // (below 2^31: component numbers and the box are 32-bit)
    const int rc = check_extents(3, {{d->ext, 0x7fffffffL, nullptr, &cells, nullptr}});
    if (rc != DLKA_OK) return rc;
    if (d->rank == 2 && d->ext[0] != 1) return DLKA_ERR_SHAPE;
    return DLKA_OK;
}

static int prep_check_box(const dlka_prep_desc *d)
{
    if (d->seg_channels < 0) return DLKA_ERR_SHAPE;
    if (d->seg_channels > DLKA_PREP_C_MAX) return DLKA_ERR_UNSUPPORTED;
    for (int ax = 0; ax < 3; ++ax)
        if (d->lo[ax] < 0 || d->hi[ax] <= d->lo[ax] || d->hi[ax] > d->ext[ax]) return DLKA_ERR_SHAPE;
    return DLKA_OK;
}

static PrepArgs prep_args(const dlka_prep_desc *d)
{
    PrepArgs a = {};
    a.rank = d->rank; a.C = d->C; a.nan0 = d->nan_to_zero ? 1 : 0; a.label = d->nonzero_label;
    a.has_seg = d->seg_channels > 0 ? 1 : 0;
    a.S = a.has_seg ? d->seg_channels : 1;
    a.N = 1;
    for (int ax = 0; ax < 3; ++ax) { a.ext[ax] = (int)d->ext[ax]; a.N *= (long)d->ext[ax]; }
    return a;
}

static unsigned prep_grid(long cells) { return (unsigned)cdivl(cells, (long)PREP_THREADS * PREP_PER); }

static int prep_stat_blocks(long cells)
{
    const long n = cdivl(cells, PREP_STAT_CHUNK);
    return (int)(n < 1 ? 1 : n > PREP_STAT_BLOCKS_MAX ? PREP_STAT_BLOCKS_MAX : n);
}

static int prep_box_pass(const unsigned char *in, const int32_t *labels, const unsigned char *flag, uint8_t *mask, int32_t *box, const PrepArgs &a,
                         hipStream_t st)
{
    DLKA_LAUNCH(dlka_prep_box_init_kernel, dim3(1), dim3(64), 0, st, (int *)box);
    DLKA_CHECK_LAUNCH();
    if (labels) {
        long plane = 1;
        for (int ax = 3 - a.rank; ax < 3; ++ax) {
            const long p = a.N / a.ext[ax];
            plane = p > plane ? p : plane;
        }
        DLKA_LAUNCH(dlka_prep_faces_kernel, dim3((unsigned)cdivl(plane, PREP_THREADS), (unsigned)(2 * a.rank)), dim3(PREP_THREADS), 0, st,
                    (const int *)labels, const_cast<unsigned char *>(flag), a);
        DLKA_CHECK_LAUNCH();
    }
    DLKA_LAUNCH(dlka_prep_fill_kernel, dim3(prep_grid(a.N)), dim3(PREP_THREADS), 0, st, in, (const int *)labels, flag, (unsigned char *)mask,
                (int *)box, a);
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}

}  // namespace dlka

using namespace dlka;

extern "C" int dlka_prep_background(const float *data, const dlka_prep_desc *d, uint8_t *background, void *stream)
{
    const int rc = prep_check(d);
    if (rc != DLKA_OK) return rc;
    if (!data || !background) return DLKA_ERR_NULL;
    const PrepArgs a = prep_args(d);
    g_prep_launches.add();
    DLKA_LAUNCH(dlka_prep_background_kernel, dim3(prep_grid(a.N)), dim3(PREP_THREADS), 0, (hipStream_t)stream, data, (unsigned char *)background,
                a.N, a.C);
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}

extern "C" size_t dlka_prep_fill_workspace_bytes(const dlka_prep_desc *d)
{
    if (prep_check(d) != DLKA_OK) return 0;
    return (size_t)prep_args(d).N + 1;    // one flag per component number 0..N
}

extern "C" int dlka_prep_fill_bbox(const uint8_t *background, const int32_t *labels, const dlka_prep_desc *d, void *workspace,
                                   size_t workspace_bytes, uint8_t *mask, int32_t *box, void *stream)
{
    const int rc = prep_check(d);
    if (rc != DLKA_OK) return rc;
    if (!background || !labels || !mask || !box) return DLKA_ERR_NULL;
    const PrepArgs a = prep_args(d);
    if (!workspace || workspace_bytes < (size_t)a.N + 1) return DLKA_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(workspace, 0, (size_t)a.N + 1, st) != hipSuccess) return DLKA_ERR_LAUNCH;
    g_prep_launches.add(3);
    return prep_box_pass(background, labels, (const unsigned char *)workspace, mask, box, a, st);
}

extern "C" int dlka_prep_mask_bbox(const uint8_t *mask, const dlka_prep_desc *d, int32_t *box, void *stream)
{
    const int rc = prep_check(d);
    if (rc != DLKA_OK) return rc;
    if (!mask || !box) return DLKA_ERR_NULL;
    g_prep_launches.add(2);
    return prep_box_pass(mask, nullptr, nullptr, nullptr, box, prep_args(d), (hipStream_t)stream);
}

extern "C" int dlka_prep_crop(const float *data, const int32_t *seg, const uint8_t *mask, const dlka_prep_desc *d, float *out, int32_t *seg_out,
                              void *stream)
{
    int rc = prep_check(d);
    if (rc == DLKA_OK) rc = prep_check_box(d);
    if (rc != DLKA_OK) return rc;
    if (!data || !out) return DLKA_ERR_NULL;
    if (seg_out && !mask) return DLKA_ERR_NULL;
    if (seg_out && d->seg_channels > 0 && !seg) return DLKA_ERR_NULL;
    if (out == data || (seg_out && seg_out == seg)) return DLKA_ERR_UNSUPPORTED;
    PrepArgs a = prep_args(d);
    a.NC = 1;
    for (int ax = 0; ax < 3; ++ax) {
        a.lo[ax] = (int)d->lo[ax];
        a.cext[ax] = (int)(d->hi[ax] - d->lo[ax]);
        a.NC *= (long)a.cext[ax];
    }
    g_prep_launches.add();
    DLKA_LAUNCH(dlka_prep_crop_kernel, dim3(prep_grid(a.NC)), dim3(PREP_THREADS), 0, (hipStream_t)stream, data, (const int *)seg,
                (const unsigned char *)mask, out, (int *)seg_out, a);
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}

extern "C" size_t dlka_prep_stats_workspace_bytes(const dlka_prep_desc *d)
{
    if (prep_check(d) != DLKA_OK) return 0;
    return (size_t)d->C * (size_t)prep_stat_blocks(prep_args(d).N) * 2 * sizeof(double);
}

extern "C" int dlka_prep_channel_stats(const float *data, const int32_t *seg, const dlka_prep_desc *d, double *table, void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    const int rc = prep_check(d);
    if (rc != DLKA_OK) return rc;
    if (!data || !seg || !table) return DLKA_ERR_NULL;
    if (!workspace || workspace_bytes < dlka_prep_stats_workspace_bytes(d) || ((uintptr_t)workspace & 7) != 0) return DLKA_ERR_WORKSPACE;
    const PrepArgs a = prep_args(d);
    const int nblk = prep_stat_blocks(a.N);
    hipStream_t st = (hipStream_t)stream;
    double *partials = (double *)workspace;
    g_prep_launches.add(4);
    for (int pass = 0; pass < 2; ++pass) {
        DLKA_LAUNCH(dlka_prep_stats_kernel, dim3((unsigned)nblk, (unsigned)a.C), dim3(PREP_THREADS), 0, st, data, (const int *)seg,
                    (const double *)table, partials, a.N, pass);
        DLKA_CHECK_LAUNCH();
        DLKA_LAUNCH(dlka_prep_stats_finish_kernel, dim3((unsigned)cdivl(a.C, PREP_THREADS)), dim3(PREP_THREADS), 0, st, (const double *)partials,
                    table, a.C, nblk, pass);
        DLKA_CHECK_LAUNCH();
    }
    return DLKA_OK;
}

extern "C" int dlka_prep_normalize(const float *data, const int32_t *seg, const dlka_prep_desc *d, const double *table, float *out, void *stream)
{
    const int rc = prep_check(d);
    if (rc != DLKA_OK) return rc;
    if (!data || !seg || !table || !out) return DLKA_ERR_NULL;
    const PrepArgs a = prep_args(d);
    g_prep_launches.add();
    DLKA_LAUNCH(dlka_prep_normalize_kernel, dim3(prep_grid(a.N), (unsigned)a.C), dim3(PREP_THREADS), 0, (hipStream_t)stream, data,
                (const int *)seg, table, out, a.N);
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}
