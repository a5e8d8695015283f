// Surface distances and overlap counts of label maps (include/dlka.h: dlka_sd_*): what medpy.metric.binary.dc / hd / hd95 / asd / assd
// compute on the host for every evaluator of the reference (2D/utils.py:50-60, 3D/d_lka_former/inference_synapse.py:11-21,
// inference_acdc.py:29-51, 3D/pancreas_code/test_util.py:130, 3D/d_lka_former/evaluation/metrics.py:314-383).
//
// A call works on K classes of two label maps of equal extents (ed, eh, ew; rank 2 has ed = 1), i.e. on M = 2 K mask pairs: pair 2c
// measures from the border of (prediction == id_c) to the border of (label == id_c), pair 2c + 1 the other way.  The masks are never
// materialised: every kernel compares the label maps' values with the class id (mask mode: value != 0).
//
//   stats     one pass over both maps per group of SD_KC classes: |a & b|, |a|, |b| and the bounding box of a | b, per class.  Reduced
//             through LDS in lane order, one partial row per workgroup, added in workgroup order by the finishing launch.  Integers throughout.
//   line      border extraction fused with the transform along the contiguous axis: a workgroup owns one line of one pair's box, marks
//             border = mask & ~erode(mask) (scipy's generate_binary_structure(rank, connectivity); cells outside the ARRAY are 0) as one
//             bit per cell in LDS (__ballot) and every lane finds the nearest set bit of its cells by count-leading / trailing-zeros over
//             the words: the exact index distance |dw| (int32, -1 = the line has no border cell).
//   axis      the transform along a strided axis as a tile of 64 outputs x 16 columns per workgroup, candidates staged through LDS in
//             chunks of 64: out(i) = min_j ((i - j) s)^2 + in(j), float64, every candidate of the line visited (no search radius).  First
//             along h, (dw sw)^2 as input; then along d, where only the cells of the OTHER pair's border (its dw == 0) are evaluated and
//             the rest get -1.  Tiles without such a cell leave at once.
//
// Exactness: min over the line of a separable sum is the lower-envelope recurrence of Felzenszwalb & Huttenlocher evaluated in full; with
// unit spacing every term is an integer below 2^53, so the squared distance is the integer scipy's feature transform arrives at.  The
// kernels return SQUARED distances; the square root is the caller's (IEEE on the host for the values a metric returns).
// Cropping to the box of a | b is exact: outside it both masks are 0, which is what the array's outside counts as, and no border cell
// lies outside it.  No atomics; every output cell is written by exactly one lane: two runs give the same bits.
#include <math.h>

#include "cl_pipeline.h"

DLKA_LAUNCH_COUNTER(g_sd_launches, dlka_sd_launch_count)

namespace dlka {

#define SD_THREADS 256
#define SD_KC 4          // classes per workgroup of the stats pass
#define SD_NQ 9          // per class: inter, |a|, |b|, lo[3], hi[3]
#define SD_TW 16         // columns (contiguous axis) of an axis-pass tile
#define SD_TO 64         // outputs along the axis per tile (4 per lane) = candidates per LDS chunk
#define SD_MAX_W 32768   // longest contiguous line: one bit per cell in LDS
#define SD_BIG 0x7fffffff

struct SdBox { int lo[3], ext[3]; long off; };   // off: cells before this class's two pairs in the per-pair buffers

struct SdArgs {
    int rank, conn, K, mask_mode;
    int ext[3];
    double s[3];
    long id[DLKA_SD_K_MAX];
    SdBox box[DLKA_SD_K_MAX];
};

template <typename L> __device__ __forceinline__ bool sd_in(const L *m, long idx, long id, int mask_mode)
{
    const long v = (long)m[idx];
    return mask_mode ? v != 0 : v == id;
}

// rows (d, h) are dealt to the workgroups of one class group round-robin; lanes stride along w
template <typename L>
__global__ __launch_bounds__(SD_THREADS) void dlka_sd_stats_kernel(const SdArgs a, const L *__restrict__ p, const L *__restrict__ q, int *__restrict__ partial)
{
    __shared__ int red[SD_KC * SD_NQ][SD_THREADS + 1];
    __shared__ int fold[SD_KC * SD_NQ][4];
    const int tid = threadIdx.x, g = blockIdx.x, G = gridDim.x, k0 = blockIdx.y * SD_KC;
    const int ed = a.ext[0], eh = a.ext[1], ew = a.ext[2];
    int acc[SD_KC][SD_NQ];
#pragma unroll
    for (int k = 0; k < SD_KC; ++k) {
        acc[k][0] = acc[k][1] = acc[k][2] = 0;
        acc[k][3] = acc[k][4] = acc[k][5] = SD_BIG;
        acc[k][6] = acc[k][7] = acc[k][8] = -1;
    }
    const long rows = (long)ed * eh;
    for (long r = g; r < rows; r += G) {
        const int d = (int)(r / eh), h = (int)(r % eh);
        for (int w = tid; w < ew; w += SD_THREADS) {
            const long idx = r * ew + w;
#pragma unroll
            for (int k = 0; k < SD_KC; ++k) {
                if (k0 + k < a.K) {
                    const bool ia = sd_in(p, idx, a.id[k0 + k], a.mask_mode), ib = sd_in(q, idx, a.id[k0 + k], a.mask_mode);
                    acc[k][0] += (ia && ib) ? 1 : 0;
                    acc[k][1] += ia ? 1 : 0;
                    acc[k][2] += ib ? 1 : 0;
                    if (ia || ib) {
                        acc[k][3] = min(acc[k][3], d); acc[k][4] = min(acc[k][4], h); acc[k][5] = min(acc[k][5], w);
                        acc[k][6] = max(acc[k][6], d); acc[k][7] = max(acc[k][7], h); acc[k][8] = max(acc[k][8], w);
                    }
                }
            }
        }
    }
    // every lane's row to LDS; 4 lanes per quantity fold 64 rows each in row order, then one lane folds the 4: two barriers, no wave operation
#pragma unroll
    for (int k = 0; k < SD_KC; ++k)
#pragma unroll
        for (int j = 0; j < SD_NQ; ++j) red[k * SD_NQ + j][tid] = acc[k][j];
    __syncthreads();
    if (tid < 4 * SD_KC * SD_NQ) {
        const int s = tid >> 2, part = tid & 3, j = s % SD_NQ;
        int v = red[s][part * 64];
        for (int i = 1; i < 64; ++i) {
            const int u = red[s][part * 64 + i];
            v = j < 3 ? v + u : (j < 6 ? (u < v ? u : v) : (u > v ? u : v));
        }
        fold[s][part] = v;
    }
    __syncthreads();
    if (tid < SD_KC * SD_NQ) {
        const int j = tid % SD_NQ;
        int v = fold[tid][0];
        for (int w = 1; w < 4; ++w) {
            const int u = fold[tid][w];
            v = j < 3 ? v + u : (j < 6 ? (u < v ? u : v) : (u > v ? u : v));
        }
        partial[((long)blockIdx.y * G + g) * (SD_KC * SD_NQ) + tid] = v;
    }
}

// stats[K][9] int64 = inter, |a|, |b|, lo d h w, hi d h w (lo > hi for a class absent from both maps)
__global__ __launch_bounds__(SD_THREADS) void dlka_sd_stats_finish_kernel(int K, int G, const int *__restrict__ partial, int64_t *__restrict__ stats)
{
    for (int t = threadIdx.x; t < K * SD_NQ; t += SD_THREADS) {
        const int k = t / SD_NQ, j = t % SD_NQ, y = k / SD_KC, s = (k % SD_KC) * SD_NQ + j;
        int64_t v = j < 3 ? 0 : (j < 6 ? SD_BIG : -1);
        for (int g = 0; g < G; ++g) {
            const int64_t u = partial[((long)y * G + g) * (SD_KC * SD_NQ) + s];
            v = j < 3 ? v + u : (j < 6 ? (u < v ? u : v) : (u > v ? u : v));
        }
        stats[t] = v;
    }
}

// border = mask & ~erode(mask) at array cell (d, h, w); the caller has checked that the cell is in the array
template <typename L>
__device__ __forceinline__ bool sd_border(const SdArgs &a, const L *m, long id, int d, int h, int w)
{
    const int ed = a.ext[0], eh = a.ext[1], ew = a.ext[2];
    const long idx = ((long)d * eh + h) * ew + w;
    if (!sd_in(m, idx, id, a.mask_mode)) return false;
    const int zlo = a.rank == 3 ? -1 : 0, zhi = a.rank == 3 ? 1 : 0;
    for (int dz = zlo; dz <= zhi; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int l1 = (dz != 0) + (dy != 0) + (dx != 0);
                if (l1 == 0 || l1 > a.conn) continue;
                const int z = d + dz, y = h + dy, x = w + dx;
                if (z < 0 || z >= ed || y < 0 || y >= eh || x < 0 || x >= ew) return true;   // border_value = 0
                if (!sd_in(m, ((long)z * eh + y) * ew + x, id, a.mask_mode)) return true;
            }
    return false;
}

// one workgroup per line (blockIdx.x over the d, h of the class's box) of one pair (blockIdx.y); dw[pair cells] int32
template <typename L>
__global__ __launch_bounds__(SD_THREADS) void dlka_sd_line_kernel(const SdArgs a, const L *__restrict__ p, const L *__restrict__ q, int *__restrict__ dw)
{
    __shared__ unsigned long long bits[SD_MAX_W / 64];
    const int tid = threadIdx.x, pair = blockIdx.y, c = pair >> 1, dir = pair & 1;
    const SdBox bx = a.box[c];
    const int bd = bx.ext[0], bh = bx.ext[1], bw = bx.ext[2];
    if ((long)blockIdx.x >= (long)bd * bh) return;
    const int d = bx.lo[0] + (int)(blockIdx.x / bh), h = bx.lo[1] + (int)(blockIdx.x % bh);
    const L *target = dir == 0 ? q : p;   // the distance is measured TO the border of the other mask
    const long id = a.id[c];
    const int nw = (bw + 63) >> 6;
    for (int c0 = 0; c0 < bw; c0 += SD_THREADS) {   // (uniform trip count: every lane takes part in the ballot)
        const int w = c0 + tid;
        const bool b = w < bw && sd_border(a, target, id, d, h, bx.lo[2] + w);
        const unsigned long long m = __ballot(b ? 1 : 0);
        if ((tid & 63) == 0 && (w >> 6) < nw) bits[w >> 6] = m;
    }
    __syncthreads();
    int *out = dw + bx.off + (long)dir * bd * bh * bw + (long)blockIdx.x * bw;
    for (int w = tid; w < bw; w += SD_THREADS) {
        const int qw = w >> 6, r = w & 63;
        const unsigned long long word = bits[qw];
        int best = SD_BIG;
        const unsigned long long left = word & ((2ull << r) - 1ull), right = word & (~0ull << r);
        if (left) best = r - (63 - __builtin_clzll(left));
        else
            for (int j = qw - 1; j >= 0; --j) {
                const unsigned long long u = bits[j];
                if (u) { best = w - (j * 64 + 63 - __builtin_clzll(u)); break; }
            }
        if (right) best = min(best, __builtin_ctzll(right) - r);
        else
            for (int j = qw + 1; j < nw; ++j) {
                const unsigned long long u = bits[j];
                if (u) { best = min(best, j * 64 + __builtin_ctzll(u) - w); break; }
            }
        out[w] = best == SD_BIG ? -1 : best;
    }
}

// axis 1: along h (FIRST: the input is dw); axis 0: along d (SAMPLE: only where the other pair's dw is 0).
// lin = ((outer * nob) + ob) * nwt + wt;  lane = (wl = tid & 15, hr = tid >> 4), outputs i = ob * 64 + hr + 16 r
template <bool FIRST, bool SAMPLE>
__global__ __launch_bounds__(SD_THREADS) void dlka_sd_axis_kernel(const SdArgs a, int axis, const int *__restrict__ dw, const double *__restrict__ in,
                                                                  double *__restrict__ out)
{
    __shared__ double cand[SD_TO][SD_TW];
    __shared__ int any;
    const int tid = threadIdx.x, pair = blockIdx.y, c = pair >> 1, dir = pair & 1;
    const SdBox bx = a.box[c];
    const int bd = bx.ext[0], bh = bx.ext[1], bw = bx.ext[2];
    const long cells = (long)bd * bh * bw;
    const int n = axis == 1 ? bh : bd, outer = axis == 1 ? bd : bh;
    const long S = axis == 1 ? bw : (long)bh * bw, outerS = axis == 1 ? (long)bh * bw : bw;
    const int nwt = (bw + SD_TW - 1) / SD_TW, nob = (n + SD_TO - 1) / SD_TO;
    const long lin = blockIdx.x;
    if (lin >= (long)outer * nob * nwt) return;
    const int wt = (int)(lin % nwt), ob = (int)((lin / nwt) % nob), o = (int)(lin / ((long)nwt * nob));
    const int wl = tid & (SD_TW - 1), hr = tid >> 4, w = wt * SD_TW + wl;
    const bool inb = w < bw;
    const long base = bx.off + (long)dir * cells + (long)o * outerS + w, other = bx.off + (long)(1 - dir) * cells + (long)o * outerS + w;
    const double s = a.s[axis], sw = a.s[2];
    int i[4];
    bool need[4];
    double acc[4];
    bool mine = false;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        i[r] = ob * SD_TO + hr + 16 * r;
        need[r] = inb && i[r] < n;
        if (SAMPLE && need[r]) need[r] = dw[other + (long)i[r] * S] == 0;
        mine = mine || need[r];
        acc[r] = INFINITY;
    }
    if (SAMPLE) {   // a tile without a border cell of the first mask has nothing to evaluate
        if (tid == 0) any = 0;
        __syncthreads();
        if (mine) any = 1;
        __syncthreads();
        if (!any) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (inb && i[r] < n) out[base + (long)i[r] * S] = -1.0;
            return;
        }
    }
    for (int c0 = 0; c0 < n; c0 += SD_TO) {
        if (c0 > 0) __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = c0 + hr + 16 * r;
            double v = INFINITY;
            if (inb && j < n) {
                if (FIRST) {
                    const int t = dw[base + (long)j * S];
                    const double x = (double)t * sw;
                    v = t < 0 ? INFINITY : x * x;
                } else {
                    v = in[base + (long)j * S];
                }
            }
            cand[hr + 16 * r][wl] = v;
        }
        __syncthreads();
        const int cnt = min(SD_TO, n - c0);
        for (int jj = 0; jj < cnt; ++jj) {
            const double f = cand[jj][wl];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double dd = (double)(i[r] - (c0 + jj)) * s;
                acc[r] = fmin(acc[r], fma(dd, dd, f));
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (inb && i[r] < n) out[base + (long)i[r] * S] = SAMPLE ? (need[r] ? acc[r] : -1.0) : acc[r];
}

static int sd_check(const dlka_sd_desc *d)
{
    if (!d) return DLKA_ERR_NULL;
    if (d->rank != 2 && d->rank != 3) return DLKA_ERR_SHAPE;
    if (d->connectivity < 1 || d->connectivity > d->rank) return DLKA_ERR_UNSUPPORTED;
    if (!label_bytes(d->label_dtype)) return DLKA_ERR_DTYPE;
    if (d->K < 1 || d->K > DLKA_SD_K_MAX) return DLKA_ERR_UNSUPPORTED;
    long cells = 1;
    // (an extent over 2^31 - 1 is a bad shape here, not an unsupported one)
    const int rc = check_extents(3, {{d->ext, 0x7fffffffL, nullptr, &cells, nullptr}},
                                 [&](int ax) { return d->ext[ax] > 0x7fffffffL ? (int)DLKA_ERR_SHAPE : (int)DLKA_OK; });
    if (rc != DLKA_OK) return rc;
    if (d->rank == 2 && d->ext[0] != 1) return DLKA_ERR_SHAPE;
    if (d->ext[2] > SD_MAX_W) return DLKA_ERR_UNSUPPORTED;
    for (int ax = 3 - d->rank; ax < 3; ++ax)
        if (!(d->spacing[ax] > 0.0) || !(d->spacing[ax] < 1e100)) return DLKA_ERR_SHAPE;
    return DLKA_OK;
}

// boxes[K][6] = lo d h w, extent d h w inside the array; an extent of 0 skips the class.  Fills the kernels' table; returns the cells of all pairs.
static int sd_boxes(const dlka_sd_desc *d, const int64_t *boxes, SdArgs &a, long *total, long *max_lines, long *max_tiles1, long *max_tiles0)
{
    long off = 0;
    *max_lines = *max_tiles1 = *max_tiles0 = 0;
    for (int k = 0; k < d->K; ++k) {
        const int64_t *b = boxes + 6 * k;
        long cells = 1;
        bool skip = false;
        for (int ax = 0; ax < 3; ++ax) {
            if (b[3 + ax] == 0) skip = true;
            if (b[ax] < 0 || b[3 + ax] < 0 || b[ax] + b[3 + ax] > d->ext[ax]) return DLKA_ERR_SHAPE;
            cells *= (long)b[3 + ax];
        }
        for (int ax = 0; ax < 3; ++ax) { a.box[k].lo[ax] = skip ? 0 : (int)b[ax]; a.box[k].ext[ax] = skip ? 0 : (int)b[3 + ax]; }
        a.box[k].off = off;
        if (skip) continue;
        off += 2 * cells;
        const long bd = b[3], bh = b[4], bw = b[5], nwt = cdivl(bw, SD_TW);
        const long lines = bd * bh, t1 = bd * cdivl(bh, SD_TO) * nwt, t0 = bh * cdivl(bd, SD_TO) * nwt;
        *max_lines = lines > *max_lines ? lines : *max_lines;
        *max_tiles1 = t1 > *max_tiles1 ? t1 : *max_tiles1;
        *max_tiles0 = t0 > *max_tiles0 ? t0 : *max_tiles0;
    }
    *total = off;
    return DLKA_OK;
}

static SdArgs sd_args(const dlka_sd_desc *d)
{
    SdArgs a = {};
    a.rank = d->rank; a.conn = d->connectivity; a.K = d->K; a.mask_mode = d->mask_mode ? 1 : 0;
    for (int ax = 0; ax < 3; ++ax) { a.ext[ax] = (int)d->ext[ax]; a.s[ax] = d->spacing[ax]; }
    for (int k = 0; k < d->K; ++k) a.id[k] = (long)d->class_id[k];
    return a;
}

static long sd_stat_groups(const dlka_sd_desc *d)
{
    const long rows = (long)d->ext[0] * d->ext[1];
    return rows < 1024 ? rows : 1024;
}

static void sd_dispatch(const dlka_sd_desc *d, const SdArgs &a, int what, const void *p, const void *q, int *ws, dim3 grid, hipStream_t st)
{
    dispatch_label(d->label_dtype, [&](auto t) -> int {
        using L = DLKA_T(t);
        g_sd_launches.add();
        if (what == 0) { auto k = dlka_sd_stats_kernel<L>; DLKA_LAUNCH(k, grid, dim3(SD_THREADS), 0, st, a, (const L *)p, (const L *)q, ws); }
        else { auto k = dlka_sd_line_kernel<L>; DLKA_LAUNCH(k, grid, dim3(SD_THREADS), 0, st, a, (const L *)p, (const L *)q, ws); }
        return DLKA_OK;
    });
}

}  // namespace dlka

using namespace dlka;

extern "C" size_t dlka_sd_stats_workspace_bytes(const dlka_sd_desc *d)
{
    if (sd_check(d) != DLKA_OK) return 0;
    return (size_t)cdivl(d->K, SD_KC) * (size_t)sd_stat_groups(d) * SD_KC * SD_NQ * sizeof(int);
}

extern "C" int dlka_sd_label_stats(const void *prediction, const void *label, const dlka_sd_desc *d, void *workspace, size_t workspace_bytes,
                                   int64_t *stats, void *stream)
{
    const int rc = sd_check(d);
    if (rc != DLKA_OK) return rc;
    if (!prediction || !label || !stats) return DLKA_ERR_NULL;
    if (!workspace || workspace_bytes < dlka_sd_stats_workspace_bytes(d)) return DLKA_ERR_WORKSPACE;
    const SdArgs a = sd_args(d);
    const long G = sd_stat_groups(d);
    hipStream_t st = (hipStream_t)stream;
    sd_dispatch(d, a, 0, prediction, label, (int *)workspace, dim3((unsigned)G, (unsigned)cdivl(d->K, SD_KC)), st);
    DLKA_CHECK_LAUNCH();
    g_sd_launches.add();
    DLKA_LAUNCH(dlka_sd_stats_finish_kernel, dim3(1), dim3(SD_THREADS), 0, st, (int)d->K, (int)G, (const int *)workspace, stats);
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}

extern "C" int64_t dlka_sd_distance_cells(const dlka_sd_desc *d, const int64_t *boxes)
{
    if (sd_check(d) != DLKA_OK || !boxes) return -1;
    SdArgs a = sd_args(d);
    long total, l, t1, t0;
    if (sd_boxes(d, boxes, a, &total, &l, &t1, &t0) != DLKA_OK) return -1;
    return (int64_t)total;
}

extern "C" int dlka_sd_distances(const void *prediction, const void *label, const dlka_sd_desc *d, const int64_t *boxes, void *workspace,
                                 size_t workspace_bytes, double *sqdist, int64_t sqdist_cells, void *stream)
{
    int rc = sd_check(d);
    if (rc != DLKA_OK) return rc;
    if (!prediction || !label || !boxes) return DLKA_ERR_NULL;
    SdArgs a = sd_args(d);
    long total, lines, tiles1, tiles0;
    rc = sd_boxes(d, boxes, a, &total, &lines, &tiles1, &tiles0);
    if (rc != DLKA_OK) return rc;
    if (total == 0) return DLKA_OK;
    if (!sqdist || sqdist_cells < total) return DLKA_ERR_SHAPE;
    if (!workspace || workspace_bytes < (size_t)total * 12) return DLKA_ERR_WORKSPACE;
    if (lines > 0x7fffffffL || tiles1 > 0x7fffffffL || tiles0 > 0x7fffffffL) return DLKA_ERR_UNSUPPORTED;
    double *g2 = (double *)workspace;                 // [total] after the pass along h
    int *dw = (int *)(g2 + total);                    // [total] index distance along w
    hipStream_t st = (hipStream_t)stream;
    const unsigned M = 2u * (unsigned)d->K;
    sd_dispatch(d, a, 1, prediction, label, dw, dim3((unsigned)lines, M), st);
    DLKA_CHECK_LAUNCH();
    g_sd_launches.add(2);
    auto along_h = dlka_sd_axis_kernel<true, false>;
    auto along_d = dlka_sd_axis_kernel<false, true>;
    DLKA_LAUNCH(along_h, dim3((unsigned)tiles1, M), dim3(SD_THREADS), 0, st, a, 1, (const int *)dw, (const double *)nullptr, g2);
    DLKA_CHECK_LAUNCH();
    DLKA_LAUNCH(along_d, dim3((unsigned)tiles0, M), dim3(SD_THREADS), 0, st, a, 0, (const int *)dw, (const double *)g2, sqdist);
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}
