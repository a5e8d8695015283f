// The 3-D trainer's batch loader (include/dlka.h: dlka_load_*): what DataLoader3D.generate_train_batch
// (3D/d_lka_former/training/dataloading/dataset_loading.py:223-379) does per batch with numpy slices and np.pad on the host, and the
// class_locations table of GenericPreprocessor._run_internal (preprocessing/preprocessing.py:333-348) that its foreground oversampling reads.
//
//   crop        ONE launch for the data and the label map of every sample of a batch.  A sample is (base pointer, three extents, the box's
//               lower corner); up to DLKA_LOAD_B_MAX of them travel by value in the kernel arguments, so no table is copied to the device
//               and no pointer array lives there.  The outputs are two flat arrays, data [B][C][patch] and seg [B][patch]; a lane owns four
//               consecutive cells of one of them and stores them with one 16-byte access.  The four cells may lie in different rows,
//               channels or samples: each finds its own source cell (the first by division, the next by carries).  A source row starts at
//               lb_z + extent products, which is 16-byte aligned only by accident: sources are read cell by cell.  Outside the case the
//               data takes the constant or, for 'edge', the nearest cell (np.pad's rule axis by axis = clamped indices); the label map
//               always takes -1.  Cells move as 32-bit words: no floating-point instruction touches them.
//   classes     all K classes in one read of the label map.  A TILE is what ONE WAVE owns: LOAD_CL_ITERS rounds of 64 consecutive cells,
//               so raster order is (tile, round, lane) and nothing crosses a wave: no LDS, no barrier.
//               (a) count: per round the wave walks the DISTINCT classes of its 64 cells (first live lane's class, __ballot of its equals,
//                   strike them out); lane k keeps class k's sum.  counts[k][tile].
//               (b) scan: one workgroup per class turns counts[k][.] into exclusive offsets in place and writes the class total.
//               (c) scatter: the same walk; a cell's rank = offset of its tile + the class's sum over the earlier rounds (lane k's register,
//                   read with __shfl) + the set bits below its lane in the ballot.  locs[base[k] + rank] = linear cell index: argwhere in
//                   raster order, fixed by the scan.  No atomic anywhere.
//               (d) gather: out[j] = the (x, y, z) of locs[base[class[j]] + rank[j]] for the ranks the host drew.
//               Two launches for the counts, two for the selection, whatever K and the extents are.
#include <cstring>

#include "cl_pipeline.h"

DLKA_LAUNCH_COUNTER(g_load_launches, dlka_load_launch_count)

namespace dlka {

#define LOAD_THREADS 256
#define LOAD_PER 4
#define LOAD_CL_ITERS 32
#define LOAD_CL_TILE (64 * LOAD_CL_ITERS)         // cells per wave
#define LOAD_CL_WAVES (LOAD_THREADS / 64)
#define LOAD_COORD_MAX (1L << 30)                 // patch extents and |lower corner|: their sum stays a 32-bit integer

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct LoadSample {
    const unsigned *base;                         // [C + 1][ext], the label map last
    int ext[3], lb[3];
};

struct LoadCropArgs {
    int B, C, edge;
    unsigned cval;                                // the constant's bits
    int patch[3];
    long P;                                       // cells of one patch
    LoadSample s[DLKA_LOAD_B_MAX];
};
static_assert(sizeof(LoadCropArgs) <= 1280, "the batch description stays well under the 4 KiB of kernel arguments");

__device__ __forceinline__ int load_clamp(int v, int n) { return v < 0 ? 0 : v >= n ? n - 1 : v; }

// one output cell: sample b, source channel ch, patch position (x, y, z)
__device__ __forceinline__ unsigned load_cell(const LoadCropArgs &a, int b, int ch, int x, int y, int z, bool is_seg)
{
    const LoadSample &s = a.s[b];
    int sx = x + s.lb[0], sy = y + s.lb[1], sz = z + s.lb[2];
    const bool inside = sx >= 0 && sx < s.ext[0] && sy >= 0 && sy < s.ext[1] && sz >= 0 && sz < s.ext[2];
    if (!inside) {
        if (is_seg) return 0xbf800000u;           // -1.0f
        if (!a.edge) return a.cval;
        sx = load_clamp(sx, s.ext[0]); sy = load_clamp(sy, s.ext[1]); sz = load_clamp(sz, s.ext[2]);
    }
    return s.base[(((long)ch * s.ext[0] + sx) * s.ext[1] + sy) * s.ext[2] + sz];
}

// quads [0, qd) belong to data, [qd, qd + qs) to seg
__global__ __launch_bounds__(LOAD_THREADS) void dlka_load_crop_kernel(unsigned *__restrict__ data, unsigned *__restrict__ seg, const LoadCropArgs a,
                                                                      long qd, long qs)
{
    long q = (long)blockIdx.x * LOAD_THREADS + threadIdx.x;
    if (q >= qd + qs) return;
    const bool is_seg = q >= qd;
    if (is_seg) q -= qd;
    const int chans = is_seg ? 1 : a.C;
    const long total = (long)a.B * chans * a.P, i0 = q * LOAD_PER;
    const int n = total - i0 < LOAD_PER ? (int)(total - i0) : LOAD_PER;
    const long yz = (long)a.patch[1] * a.patch[2];
    long rest = i0;
    int b = (int)(rest / (chans * a.P));
    rest -= (long)b * chans * a.P;
    int c = (int)(rest / a.P);
    rest -= (long)c * a.P;
    int x = (int)(rest / yz);
    rest -= (long)x * yz;
    int y = (int)(rest / a.patch[2]), z = (int)(rest - (long)y * a.patch[2]);
    unsigned v[LOAD_PER] = {0u, 0u, 0u, 0u};
    for (int k = 0; k < n; ++k) {
        v[k] = load_cell(a, b, is_seg ? a.C : c, x, y, z, is_seg);
        if (++z == a.patch[2]) {
            z = 0;
            if (++y == a.patch[1]) {
                y = 0;
                if (++x == a.patch[0]) {
                    x = 0;
                    if (++c == chans) { c = 0; ++b; }
                }
            }
        }
    }
    unsigned *o = (is_seg ? seg : data) + i0;
    if (n == LOAD_PER && ((uintptr_t)o & 15) == 0) *reinterpret_cast<u32x4 *>(o) = u32x4{v[0], v[1], v[2], v[3]};
    else
        for (int k = 0; k < n; ++k) o[k] = v[k];
}

// ---- class locations ------------------------------------------------------------------------------------------------------------------------------
struct LoadClassArgs {
    int K;
    int ext[3];
    long N, T;                                    // cells, tiles
    int cls[DLKA_LOAD_K_MAX];
    int total[DLKA_LOAD_K_MAX], base[DLKA_LOAD_K_MAX];   // (c), (d) only
};

__device__ __forceinline__ bool load_is(float v, int c) { return v == (float)c; }
__device__ __forceinline__ bool load_is(int v, int c) { return v == c; }

// the slot of cell i's label in cls[], -1 for a label that is not listed or a cell past the end
template <typename L> __device__ __forceinline__ int load_slot(const L *__restrict__ seg, const LoadClassArgs &a, long i)
{
    int slot = -1;
    if (i < a.N) {
        const L v = seg[i];
        for (int k = 0; k < a.K; ++k)
            if (load_is(v, a.cls[k])) slot = k;
    }
    return slot;
}

// (a) counts[k * T + tile]
template <typename L>
__global__ __launch_bounds__(LOAD_THREADS) void dlka_load_class_count_kernel(const L *__restrict__ seg, int *__restrict__ counts, const LoadClassArgs a)
{
    const int lane = (int)threadIdx.x & 63;
    const long tile = (long)blockIdx.x * LOAD_CL_WAVES + ((int)threadIdx.x >> 6);
    if (tile >= a.T) return;                      // (the whole wave)
    int sum = 0;                                  // lane k: class k
    for (int it = 0; it < LOAD_CL_ITERS; ++it) {
        const int slot = load_slot(seg, a, tile * LOAD_CL_TILE + it * 64 + lane);
        unsigned long long live = __ballot(slot >= 0 ? 1 : 0);
        while (live) {
            const int k = __shfl(slot, __builtin_ctzll(live));
            const unsigned long long m = __ballot(slot == k ? 1 : 0);
            if (lane == k) sum += __popcll(m);
            live &= ~m;
        }
    }
    if (lane < a.K) counts[(long)lane * a.T + tile] = sum;
}

// (b) blockIdx.x = class: counts[k][.] -> exclusive offsets, totals[k]
__global__ __launch_bounds__(LOAD_THREADS) void dlka_load_class_scan_kernel(int *__restrict__ counts, int *__restrict__ totals, long T)
{
    __shared__ int sh[LOAD_THREADS];
    const int tid = (int)threadIdx.x;
    int *c = counts + (long)blockIdx.x * T;
    const long seg = cdivl(T, LOAD_THREADS), lo = tid * seg, hi = lo + seg < T ? lo + seg : T;
    int s = 0;
    for (long i = lo; i < hi; ++i) s += c[i];
    sh[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < LOAD_THREADS; ++t) {
            const int v = sh[t];
            sh[t] = run;
            run += v;
        }
        totals[blockIdx.x] = run;
    }
    __syncthreads();
    int run = sh[tid];
    for (long i = lo; i < hi; ++i) {
        const int v = c[i];
        c[i] = run;
        run += v;
    }
}

// (c) locs[base[k] + rank] = cell
template <typename L>
__global__ __launch_bounds__(LOAD_THREADS) void dlka_load_class_scatter_kernel(const L *__restrict__ seg, const int *__restrict__ offsets,
                                                                               int *__restrict__ locs, const LoadClassArgs a)
{
    const int lane = (int)threadIdx.x & 63;
    const long tile = (long)blockIdx.x * LOAD_CL_WAVES + ((int)threadIdx.x >> 6);
    if (tile >= a.T) return;
    int run = lane < a.K ? offsets[(long)lane * a.T + tile] : 0;   // lane k: class k's cells before this round
    for (int it = 0; it < LOAD_CL_ITERS; ++it) {
        const long i = tile * LOAD_CL_TILE + it * 64 + lane;
        const int slot = load_slot(seg, a, i);
        unsigned long long live = __ballot(slot >= 0 ? 1 : 0);
        while (live) {
            const int k = __shfl(slot, __builtin_ctzll(live));
            const unsigned long long m = __ballot(slot == k ? 1 : 0);
            const int before = __shfl(run, k);
            if (slot == k) {
                const int rank = before + __popcll(m & ((1ull << lane) - 1ull));
                if (rank < a.total[k]) locs[(long)a.base[k] + rank] = (int)i;   // (totals that do not belong to this map write nothing outside)
            }
            if (lane == k) run += __popcll(m);
            live &= ~m;
        }
    }
}

// (d) out[j] = (x, y, z) of the rank[j]-th cell of class slot[j]; (-1, -1, -1) for a slot or rank that does not exist
__global__ __launch_bounds__(LOAD_THREADS) void dlka_load_class_gather_kernel(const int *__restrict__ locs, const int *__restrict__ sel_slot,
                                                                              const int *__restrict__ sel_rank, int *__restrict__ out, long M,
                                                                              const LoadClassArgs a)
{
    const long j = (long)blockIdx.x * LOAD_THREADS + threadIdx.x;
    if (j >= M) return;
    const int k = sel_slot[j], r = sel_rank[j];
    int x = -1, y = -1, z = -1;
    if (k >= 0 && k < a.K && r >= 0 && r < a.total[k]) {
        const int lin = locs[(long)a.base[k] + r];
        const int yz = a.ext[1] * a.ext[2];       // (below 2^31 with the whole map)
        x = lin / yz;
        const int rest = lin - x * yz;
        y = rest / a.ext[2];
        z = rest - y * a.ext[2];
    }
    out[3 * j] = x; out[3 * j + 1] = y; out[3 * j + 2] = z;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------
static int load_crop_check(const dlka_load_crop_desc *d, LoadCropArgs &a)
{
    if (!d) return DLKA_ERR_NULL;
    if (d->B < 1 || d->C < 1) return DLKA_ERR_SHAPE;
    if (d->B > DLKA_LOAD_B_MAX) return DLKA_ERR_UNSUPPORTED;
    if (d->mode != DLKA_LOAD_CONSTANT && d->mode != DLKA_LOAD_EDGE) return DLKA_ERR_UNSUPPORTED;
    a = LoadCropArgs{};
    a.B = d->B; a.C = d->C; a.edge = d->mode == DLKA_LOAD_EDGE ? 1 : 0;
    memcpy(&a.cval, &d->constant, sizeof(unsigned));
    long cells = 1;
    int rc = check_extents(3, {{d->patch, LOAD_COORD_MAX, a.patch, &cells, nullptr}});
    if (rc != DLKA_OK) return rc;
    a.P = cells;
    if ((double)a.P * (double)(a.C + 1) * (double)a.B >= 9.0e15) return DLKA_ERR_UNSUPPORTED;
    for (int b = 0; b < d->B; ++b) {
        const dlka_load_sample &s = d->sample[b];
        long n = 1;                               // (a case of 2^31 cells per channel or more is refused: DLKA_ERR_UNSUPPORTED)
        rc = check_extents(3, {{s.ext, 0x7fffffffL, a.s[b].ext, &n, nullptr}});
        if (rc != DLKA_OK) return rc;
        for (int ax = 0; ax < 3; ++ax) {
            if (s.lb[ax] < -LOAD_COORD_MAX || s.lb[ax] > LOAD_COORD_MAX) return DLKA_ERR_UNSUPPORTED;
            a.s[b].lb[ax] = (int)s.lb[ax];
        }
    }
    for (int b = 0; b < d->B; ++b) {
        if (!d->sample[b].data) return DLKA_ERR_NULL;
        a.s[b].base = (const unsigned *)d->sample[b].data;
    }
    return DLKA_OK;
}

static int load_class_check(const dlka_load_classes_desc *d, LoadClassArgs &a)
{
    if (!d) return DLKA_ERR_NULL;
    if (d->K < 1) return DLKA_ERR_SHAPE;
    if (d->K > DLKA_LOAD_K_MAX) return DLKA_ERR_UNSUPPORTED;
    if (d->dtype != DLKA_LOAD_F32 && d->dtype != DLKA_LOAD_I32) return DLKA_ERR_DTYPE;
    a = LoadClassArgs{};
    a.K = d->K;
    long cells = 1;
    const int rc = check_extents(3, {{d->ext, 0x7fffffffL, a.ext, &cells, nullptr}});
    if (rc != DLKA_OK) return rc;
    a.N = cells;
    a.T = cdivl(cells, LOAD_CL_TILE);
    for (int k = 0; k < d->K; ++k) {
        if (d->class_id[k] < -(1L << 24) || d->class_id[k] > (1L << 24)) return DLKA_ERR_UNSUPPORTED;   // (exact as float32)
        for (int j = 0; j < k; ++j)
            if (d->class_id[j] == d->class_id[k]) return DLKA_ERR_SHAPE;
        a.cls[k] = (int)d->class_id[k];
    }
    return DLKA_OK;
}

static unsigned load_class_grid(const LoadClassArgs &a) { return (unsigned)cdivl(a.T, LOAD_CL_WAVES); }

}  // namespace dlka

using namespace dlka;

extern "C" int dlka_load_crop_batch(const dlka_load_crop_desc *d, float *data, float *seg, void *stream)
{
    LoadCropArgs a;
    const int rc = load_crop_check(d, a);
    if (rc != DLKA_OK) return rc;
    if (!data || !seg) return DLKA_ERR_NULL;
    const long qd = cdivl((long)a.B * a.C * a.P, LOAD_PER), qs = cdivl((long)a.B * a.P, LOAD_PER);
    const long blocks = cdivl(qd + qs, LOAD_THREADS);
    if (blocks > 0x7fffffffL) return DLKA_ERR_UNSUPPORTED;
    g_load_launches.add();
    DLKA_LAUNCH(dlka_load_crop_kernel, dim3((unsigned)blocks), dim3(LOAD_THREADS), 0, (hipStream_t)stream, (unsigned *)data, (unsigned *)seg, a,
                qd, qs);
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}

extern "C" size_t dlka_load_counts_workspace_bytes(const dlka_load_classes_desc *d)
{
    LoadClassArgs a;
    if (load_class_check(d, a) != DLKA_OK) return 0;
    return (size_t)a.K * (size_t)a.T * sizeof(int);
}

extern "C" int dlka_load_class_counts(const void *seg, const dlka_load_classes_desc *d, void *workspace, size_t workspace_bytes, int32_t *totals,
                                      void *stream)
{
    LoadClassArgs a;
    const int rc = load_class_check(d, a);
    if (rc != DLKA_OK) return rc;
    if (!seg || !totals) return DLKA_ERR_NULL;
    if (!workspace || workspace_bytes < dlka_load_counts_workspace_bytes(d) || ((uintptr_t)workspace & 3) != 0) return DLKA_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int *counts = (int *)workspace;
    g_load_launches.add(2);
    if (d->dtype == DLKA_LOAD_F32)
        DLKA_LAUNCH(dlka_load_class_count_kernel<float>, dim3(load_class_grid(a)), dim3(LOAD_THREADS), 0, st, (const float *)seg, counts, a);
    else
        DLKA_LAUNCH(dlka_load_class_count_kernel<int>, dim3(load_class_grid(a)), dim3(LOAD_THREADS), 0, st, (const int *)seg, counts, a);
    DLKA_CHECK_LAUNCH();
    DLKA_LAUNCH(dlka_load_class_scan_kernel, dim3((unsigned)a.K), dim3(LOAD_THREADS), 0, st, counts, (int *)totals, a.T);
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}

// totals -> a.total, a.base; the sum, or -1 for totals no map of these extents can have
static long load_class_totals(const int64_t *totals, LoadClassArgs &a)
{
    long sum = 0;
    for (int k = 0; k < a.K; ++k) {
        if (totals[k] < 0 || totals[k] > a.N) return -1;
        a.total[k] = (int)totals[k];
        a.base[k] = (int)sum;
        sum += totals[k];
        if (sum > a.N) return -1;
    }
    return sum;
}

extern "C" size_t dlka_load_select_workspace_bytes(const dlka_load_classes_desc *d, const int64_t *totals)
{
    LoadClassArgs a;
    if (!totals || load_class_check(d, a) != DLKA_OK) return 0;
    const long sum = load_class_totals(totals, a);
    return sum < 0 ? 0 : (size_t)(sum > 0 ? sum : 1) * sizeof(int);
}

extern "C" int dlka_load_class_select(const void *seg, const dlka_load_classes_desc *d, const void *offsets, size_t offsets_bytes,
                                      const int64_t *totals, void *workspace, size_t workspace_bytes, const int32_t *sel_slot,
                                      const int32_t *sel_rank, int64_t count, int32_t *out, void *stream)
{
    LoadClassArgs a;
    const int rc = load_class_check(d, a);
    if (rc != DLKA_OK) return rc;
    if (!seg || !totals || !sel_slot || !sel_rank || !out) return DLKA_ERR_NULL;
    if (count < 1) return DLKA_ERR_SHAPE;
    if (count > 0x7fffffffL / 3) return DLKA_ERR_UNSUPPORTED;
    if (load_class_totals(totals, a) < 0) return DLKA_ERR_SHAPE;
    if (!offsets || offsets_bytes < dlka_load_counts_workspace_bytes(d) || ((uintptr_t)offsets & 3) != 0) return DLKA_ERR_WORKSPACE;
    if (!workspace || workspace_bytes < dlka_load_select_workspace_bytes(d, totals) || ((uintptr_t)workspace & 3) != 0) return DLKA_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int *locs = (int *)workspace;
    g_load_launches.add(2);
    if (d->dtype == DLKA_LOAD_F32)
        DLKA_LAUNCH(dlka_load_class_scatter_kernel<float>, dim3(load_class_grid(a)), dim3(LOAD_THREADS), 0, st, (const float *)seg,
                    (const int *)offsets, locs, a);
    else
        DLKA_LAUNCH(dlka_load_class_scatter_kernel<int>, dim3(load_class_grid(a)), dim3(LOAD_THREADS), 0, st, (const int *)seg,
                    (const int *)offsets, locs, a);
    DLKA_CHECK_LAUNCH();
    DLKA_LAUNCH(dlka_load_class_gather_kernel, dim3((unsigned)cdivl(count, LOAD_THREADS)), dim3(LOAD_THREADS), 0, st, (const int *)locs,
                (const int *)sel_slot, (const int *)sel_rank, (int *)out, (long)count, a);
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}
