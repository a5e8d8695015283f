// The dataset fingerprint (include/dlka.h: dlka_dstats_*): the intensity statistics DatasetAnalyzer
// (3D/d_lka_former/experiment_planning/DatasetAnalyzer.py:161-223) computes on the host from `modality[mask][::10]` of every case with
// np.median / np.mean / np.std / np.min / np.max / np.percentile, and the np.unique of a label map (:76-79).
//
//   sample      modality[seg > 0][::step] of up to DLKA_PREP_C_MAX modalities that share ONE pass over the label map.  A TILE is what one wave
//               owns: DS_ITERS rounds of 64 lanes x 4 consecutive cells, so raster order is (tile, round, lane, cell) and nothing crosses a
//               wave: no LDS, no barrier (the class_locations scheme of cl_dataload.hip).
//               (a) count: four __ballot per round (one per cell of the quad), popcounts summed: counts[tile].
//               (b) scan: one workgroup turns counts[.] into exclusive offsets in place and writes the total.
//               (c) sample: a cell's rank r = offset of its tile + the foreground cells of the earlier rounds + the set ballot bits of the
//                   lanes below + its own earlier cells.  r % step == 0 stores the cell of every modality to out[c][offset + r / step]: the
//                   caller's concatenation buffer is written in place, case after case.  The label map is read by (a) and by (c), the
//                   volume by (c) alone, and only the quads that hold a sampled cell.
//   moments     count, mean and population sd in float64, two passes (the mean, then the squared deviations about it): lane stride, wave by
//               __shfl_down, the workgroup's waves and then the workgroups in index order (prep_channel_stats of cl_preprocess.hip).  NaNs are
//               counted in pass 0; they make the mean and the sd NaN, as numpy's.
//   select      the k-th smallest for up to DLKA_DSTATS_RANKS_MAX ranks at once: a radix select over the order-preserving key of a float32
//               (ds_key), 4 passes of 8 bits, most significant first.  A pass is (hist) one LDS histogram per workgroup and still-distinct
//               prefix, folded with integer atomics into 256 global bins per prefix, and (pick) one workgroup that walks each rank's bins,
//               appends the bin to the rank's prefix, keeps the residual rank inside the bin and regroups the ranks by prefix.  The buffer is
//               never rewritten: it is read four times.  All state lives on the device; nothing is read back between passes.
//   labels      the presence bitmap of the values -1 .. 255 of a label map (atomicOr, LDS then global) and a flag for any other value.
//
// Determinism: integer atomics only (their sums and ORs do not depend on the order they land in); the float64 sums are folded in a fixed order
// without atomics.  Phases are separate launches; no lane waits for another lane's write.
#include "cl_pipeline.h"

DLKA_LAUNCH_COUNTER(g_dstats_launches, dlka_dstats_launch_count)

namespace dlka {

#define DS_THREADS 256
#define DS_PER 4
#define DS_WAVES (DS_THREADS / 64)
#define DS_ITERS 8
#define DS_TILE (64 * DS_PER * DS_ITERS)          // cells per wave
#define DS_CHUNK 16384L                           // elements per workgroup of the moments / histograms until DS_BLOCKS_MAX workgroups are in use
#define DS_BLOCKS_MAX 1024
#define DS_R DLKA_DSTATS_RANKS_MAX
#define DS_FLAG_WORD (DLKA_DSTATS_LABEL_WORDS - 1)

typedef int ds_i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned ds_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long ds_u64;

__device__ __forceinline__ bool ds_aligned(const void *p) { return ((uintptr_t)p & 15) == 0; }

// ---- foreground sample --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool ds_fg(float v) { return v > 0.f; }          // (a NaN label is no foreground)
__device__ __forceinline__ bool ds_fg(int v) { return v > 0; }
__device__ __forceinline__ void ds_quad(const float *p, float *v)
{
    const f32x4 q = *reinterpret_cast<const f32x4 *>(p);
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
}
__device__ __forceinline__ void ds_quad(const int *p, int *v)
{
    const ds_i32x4 q = *reinterpret_cast<const ds_i32x4 *>(p);
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
}

// bit k: cell i0 + k is foreground (cells past the end are not)
template <typename L> __device__ __forceinline__ unsigned ds_fg_mask(const L *__restrict__ seg, long i0, long N)
{
    if (i0 >= N) return 0u;
    L v[DS_PER] = {};
    const int n = N - i0 < DS_PER ? (int)(N - i0) : DS_PER;
    if (n == DS_PER && ds_aligned(seg + i0)) ds_quad(seg + i0, v);
    else
        for (int k = 0; k < n; ++k) v[k] = seg[i0 + k];
    unsigned m = 0u;
    for (int k = 0; k < n; ++k) m |= ds_fg(v[k]) ? 1u << k : 0u;
    return m;
}

// (a) counts[tile]
template <typename L>
__global__ __launch_bounds__(DS_THREADS) void dlka_dstats_fg_count_kernel(const L *__restrict__ seg, int *__restrict__ counts, long N, long T)
{
    const int lane = (int)threadIdx.x & 63;
    const long tile = (long)blockIdx.x * DS_WAVES + ((int)threadIdx.x >> 6);
    if (tile >= T) return;                        // (the whole wave)
    int sum = 0;
    for (int it = 0; it < DS_ITERS; ++it) {
        const unsigned m = ds_fg_mask(seg, tile * DS_TILE + (long)(it * 64 + lane) * DS_PER, N);
        for (int k = 0; k < DS_PER; ++k) sum += __popcll(__ballot((int)((m >> k) & 1u)));
    }
    if (lane == 0) counts[tile] = sum;
}

// (b) one workgroup: counts[.] -> exclusive offsets, *total
__global__ __launch_bounds__(DS_THREADS) void dlka_dstats_fg_scan_kernel(int *__restrict__ counts, long long *__restrict__ total, long T)
{
    __shared__ int sh[DS_THREADS];
    const int tid = (int)threadIdx.x;
    const long seg = cdivl(T, DS_THREADS), lo = tid * seg, hi = lo + seg < T ? lo + seg : T;
    int s = 0;
    for (long i = lo; i < hi; ++i) s += counts[i];
    sh[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < DS_THREADS; ++t) {
            const int v = sh[t];
            sh[t] = run;
            run += v;
        }
        *total = run;
    }
    __syncthreads();
    int run = sh[tid];
    for (long i = lo; i < hi; ++i) {
        const int v = counts[i];
        counts[i] = run;
        run += v;
    }
}

struct DsSampleArgs {
    int C;
    unsigned step;
    long N, T, out_count, out_stride, out_offset;
};

// (c) out[c * out_stride + out_offset + r / step] = data[c][cell] for the foreground cells of rank r with r % step == 0 and r / step < out_count
template <typename L>
__global__ __launch_bounds__(DS_THREADS) void dlka_dstats_fg_sample_kernel(const float *__restrict__ data, const L *__restrict__ seg,
                                                                           const int *__restrict__ offsets, float *__restrict__ out,
                                                                           const DsSampleArgs a)
{
    const int lane = (int)threadIdx.x & 63;
    const long tile = (long)blockIdx.x * DS_WAVES + ((int)threadIdx.x >> 6);
    if (tile >= a.T) return;
    const ds_u64 below = (1ull << lane) - 1ull;
    unsigned run = (unsigned)offsets[tile];       // foreground cells before this round (the same in every lane)
    for (int it = 0; it < DS_ITERS; ++it) {
        const long i0 = tile * DS_TILE + (long)(it * 64 + lane) * DS_PER;
        const unsigned m = ds_fg_mask(seg, i0, a.N);
        unsigned before = 0u, all = 0u;
        for (int k = 0; k < DS_PER; ++k) {
            const ds_u64 b = __ballot((int)((m >> k) & 1u));
            before += (unsigned)__popcll(b & below);
            all += (unsigned)__popcll(b);
        }
        if (m) {
            const unsigned r = run + before;
            unsigned q = r / a.step, rem = r - q * a.step, take = 0u;
            long slot[DS_PER] = {0, 0, 0, 0};
            for (int k = 0; k < DS_PER; ++k) {
                if (!((m >> k) & 1u)) continue;
                if (rem == 0u && (long)q < a.out_count) {
                    take |= 1u << k;
                    slot[k] = (long)q;
                }
                if (++rem == a.step) { rem = 0u; ++q; }
            }
            if (take) {
                for (int c = 0; c < a.C; ++c) {
                    const float *p = data + (long)c * a.N + i0;
                    float *o = out + (long)c * a.out_stride + a.out_offset;
                    if (i0 + DS_PER <= a.N && ds_aligned(p)) {
                        float v[DS_PER];
                        ds_quad(p, v);
                        for (int k = 0; k < DS_PER; ++k)
                            if ((take >> k) & 1u) o[slot[k]] = v[k];
                    } else {
                        for (int k = 0; k < DS_PER; ++k)
                            if ((take >> k) & 1u) o[slot[k]] = p[k];
                    }
                }
            }
        }
        run += all;
    }
}

// ---- moments ------------------------------------------------------------------------------------------------------------------------------------
// result[4] = count, mean, sd, NaNs.  pass 0: partials[workgroup] = (sum, NaNs); pass 1: (sum of squares about result[1], unused)
__global__ __launch_bounds__(DS_THREADS) void dlka_dstats_moments_kernel(const float *__restrict__ x, const double *__restrict__ result,
                                                                         double *__restrict__ partials, long n, int pass)
{
#pragma clang fp contract(off)
    __shared__ double sh[2][DS_WAVES];
    const int nblk = (int)gridDim.x, j = (int)blockIdx.x, tid = (int)threadIdx.x;
    const double mean = pass ? result[1] : 0.0;
    const long chunk = cdivl(cdivl(n, nblk), DS_PER) * DS_PER, lo = j * chunk, hi = lo + chunk < n ? lo + chunk : n;
    double s = 0.0, nans = 0.0;
    for (long i = lo + (long)tid * DS_PER; i < hi; i += (long)DS_THREADS * DS_PER) {
        const int m = hi - i < DS_PER ? (int)(hi - i) : DS_PER;
        float v[DS_PER] = {0.f, 0.f, 0.f, 0.f};
        if (m == DS_PER && ds_aligned(x + i)) ds_quad(x + i, v);
        else
            for (int k = 0; k < m; ++k) v[k] = x[i + k];
        for (int k = 0; k < m; ++k) {
            const double dv = (double)v[k] - mean;
            s = s + (pass ? dv * dv : dv);
            if (v[k] != v[k]) nans = nans + 1.0;
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        s = s + __shfl_down(s, off);
        nans = nans + __shfl_down(nans, off);
    }
    if ((tid & 63) == 0) {
        sh[0][tid >> 6] = s;
        sh[1][tid >> 6] = nans;
    }
    __syncthreads();
    if (tid == 0) {
        for (int wv = 1; wv < DS_WAVES; ++wv) {
            s = s + sh[0][wv];
            nans = nans + sh[1][wv];
        }
        partials[2 * j] = s;
        partials[2 * j + 1] = nans;
    }
}

// the final workgroup: the partials in index order
__global__ void dlka_dstats_moments_finish_kernel(const double *__restrict__ partials, double *__restrict__ result, long n, int nblk, int pass)
{
#pragma clang fp contract(off)
    if (threadIdx.x != 0) return;
    double s = partials[0], nans = partials[1];
    for (int j = 1; j < nblk; ++j) {
        s = s + partials[2 * j];
        nans = nans + partials[2 * j + 1];
    }
    if (pass) {
        result[2] = sqrt(s / (double)n);
    } else {
        result[0] = (double)n;
        result[1] = s / (double)n;
        result[3] = nans;
    }
}

// ---- exact selection ----------------------------------------------------------------------------------------------------------------------------
// The key of a float32: unsigned order of the keys = numeric order of the values, -0.0 and +0.0 being one value (the key of +0.0).
__device__ __forceinline__ unsigned ds_key(unsigned u)
{
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned ds_unkey(unsigned k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }
__device__ __forceinline__ bool ds_is_nan(unsigned u) { return (u & 0x7fffffffu) > 0x7f800000u; }

struct DsSelState {
    ds_u64 hist[DS_R][256];                       // slot s: the bins of the ranks whose prefix is prefix[s]
    ds_u64 residual[DS_R];                        // rank j among the values that share prefix[j]
    ds_u64 nans;
    unsigned prefix[DS_R];                        // the key bits found so far, right-aligned
    int slot[DS_R];                               // the first rank with rank j's prefix; -1: rank j lies beyond the values that are no NaN
    int active[DS_R];                             // slot s is some rank's
};

struct DsRanks {
    int n;
    ds_u64 r[DS_R];
};

__global__ __launch_bounds__(DS_THREADS) void dlka_dstats_select_init_kernel(DsSelState *__restrict__ st, const DsRanks ranks)
{
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < DS_R * 256; i += DS_THREADS) st->hist[i >> 8][i & 255] = 0ull;
    if (tid < DS_R) {
        st->residual[tid] = tid < ranks.n ? ranks.r[tid] : 0ull;
        st->prefix[tid] = 0u;
        st->slot[tid] = tid < ranks.n ? 0 : -1;   // (before the first pass every rank shares the empty prefix)
        st->active[tid] = tid == 0 ? 1 : 0;
    }
    if (tid == 0) st->nans = 0ull;
}

__global__ __launch_bounds__(DS_THREADS) void dlka_dstats_select_hist_kernel(const float *__restrict__ x, long n, DsSelState *__restrict__ st, int pass)
{
    __shared__ int lh[DS_R][256];
    __shared__ int lnan;
    const int nblk = (int)gridDim.x, j = (int)blockIdx.x, tid = (int)threadIdx.x;
    unsigned pre[DS_R];
    unsigned act = 0u;
    for (int s = 0; s < DS_R; ++s) {
        pre[s] = st->prefix[s];
        act |= st->active[s] ? 1u << s : 0u;
    }
    for (int i = tid; i < DS_R * 256; i += DS_THREADS) lh[i >> 8][i & 255] = 0;
    if (tid == 0) lnan = 0;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const unsigned *xb = reinterpret_cast<const unsigned *>(x);
    const long chunk = cdivl(cdivl(n, nblk), DS_PER) * DS_PER, lo = j * chunk, hi = lo + chunk < n ? lo + chunk : n;
    int nans = 0;
    for (long i = lo + (long)tid * DS_PER; i < hi; i += (long)DS_THREADS * DS_PER) {
        const int m = hi - i < DS_PER ? (int)(hi - i) : DS_PER;
        unsigned v[DS_PER] = {0u, 0u, 0u, 0u};
        if (m == DS_PER && ds_aligned(xb + i)) {
            const ds_u32x4 q = *reinterpret_cast<const ds_u32x4 *>(xb + i);
            v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
        } else {
            for (int k = 0; k < m; ++k) v[k] = xb[i + k];
        }
        for (int k = 0; k < m; ++k) {
            if (ds_is_nan(v[k])) {
                ++nans;
                continue;
            }
            const unsigned key = ds_key(v[k]);
            const unsigned high = pass ? key >> (shift + 8) : 0u;
            const int bin = (int)((key >> shift) & 255u);
            for (int s = 0; s < DS_R; ++s)
                if (((act >> s) & 1u) && high == pre[s]) atomicAdd(&lh[s][bin], 1);
        }
    }
    if (pass == 0 && nans) atomicAdd(&lnan, nans);
    __syncthreads();
    for (int i = tid; i < DS_R * 256; i += DS_THREADS) {
        const int c = lh[i >> 8][i & 255];
        if (c) atomicAdd(&st->hist[i >> 8][i & 255], (ds_u64)c);
    }
    if (tid == 0 && lnan) atomicAdd(&st->nans, (ds_u64)lnan);
}

// one workgroup: lane j walks the bins of rank j
__global__ __launch_bounds__(DS_THREADS) void dlka_dstats_select_pick_kernel(DsSelState *__restrict__ st, int n_ranks, int pass,
                                                                             float *__restrict__ values, long long *__restrict__ nan_count)
{
    __shared__ int sbin[DS_R];
    __shared__ ds_u64 sres[DS_R];
    const int tid = (int)threadIdx.x;
    if (tid < DS_R) {
        int bin = -1;
        ds_u64 res = 0ull;
        const int s = tid < n_ranks ? st->slot[tid] : -1;
        if (s >= 0) {
            const ds_u64 r = st->residual[tid];
            ds_u64 cum = 0ull;
            for (int b = 0; b < 256; ++b) {
                const ds_u64 h = st->hist[s][b];
                if (r < cum + h) {
                    bin = b;
                    res = r - cum;
                    break;
                }
                cum += h;
            }
        }
        sbin[tid] = bin;
        sres[tid] = res;
    }
    __syncthreads();                              // (every bin has been read)
    for (int i = tid; i < DS_R * 256; i += DS_THREADS) st->hist[i >> 8][i & 255] = 0ull;
    if (tid != 0) return;
    for (int j = 0; j < DS_R; ++j) {
        st->active[j] = 0;
        if (sbin[j] < 0) {
            st->slot[j] = -1;
            continue;
        }
        st->prefix[j] = (st->prefix[j] << 8) | (unsigned)sbin[j];
        st->residual[j] = sres[j];
    }
    for (int j = 0; j < DS_R; ++j) {
        if (sbin[j] < 0) continue;
        int first = j;
        for (int i = j - 1; i >= 0; --i)
            if (sbin[i] >= 0 && st->prefix[i] == st->prefix[j]) first = i;
        st->slot[j] = first;
        st->active[first] = 1;
    }
    if (pass == 3) {
        for (int j = 0; j < n_ranks; ++j) values[j] = __uint_as_float(sbin[j] < 0 ? 0x7fc00000u : ds_unkey(st->prefix[j]));
        if (nan_count) *nan_count = (long long)st->nans;
    }
}

// ---- unique labels ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ds_atomic_or(unsigned *p, unsigned v)
{
#if defined(HIPEMU)
    __atomic_fetch_or(p, v, __ATOMIC_RELAXED);
#else
    atomicOr(p, v);
#endif
}
// the bit number of a label: value - DLKA_DSTATS_LABEL_MIN, or -1 for a value outside DLKA_DSTATS_LABEL_MIN .. DLKA_DSTATS_LABEL_MAX
__device__ __forceinline__ int ds_label_code(int v)
{
    return v < DLKA_DSTATS_LABEL_MIN || v > DLKA_DSTATS_LABEL_MAX ? -1 : v - DLKA_DSTATS_LABEL_MIN;
}
__device__ __forceinline__ int ds_label_code(float v)   // (a NaN, an infinity and a value that is no integer lie outside)
{
    if (!(v >= (float)DLKA_DSTATS_LABEL_MIN && v <= (float)DLKA_DSTATS_LABEL_MAX)) return -1;
    const int i = (int)v;
    return (float)i == v ? i - DLKA_DSTATS_LABEL_MIN : -1;
}

// bitmap[DLKA_DSTATS_LABEL_WORDS]: bit (value + 1) of the first words, the last word != 0 for a value outside the range
template <typename L>
__global__ __launch_bounds__(DS_THREADS) void dlka_dstats_labels_kernel(const L *__restrict__ seg, long N, unsigned *__restrict__ bitmap)
{
    __shared__ unsigned lb[DLKA_DSTATS_LABEL_WORDS];
    const int tid = (int)threadIdx.x;
    if (tid < DLKA_DSTATS_LABEL_WORDS) lb[tid] = 0u;
    __syncthreads();
    int last = -2;                                // (a lane repeats no OR for a run of one label)
    for (long i0 = ((long)blockIdx.x * DS_THREADS + tid) * DS_PER; i0 < N; i0 += (long)gridDim.x * DS_THREADS * DS_PER) {
        const int n = N - i0 < DS_PER ? (int)(N - i0) : DS_PER;
        L v[DS_PER] = {};
        if (n == DS_PER && ds_aligned(seg + i0)) ds_quad(seg + i0, v);
        else
            for (int k = 0; k < n; ++k) v[k] = seg[i0 + k];
        for (int k = 0; k < n; ++k) {
            const int code = ds_label_code(v[k]);
            if (code == last) continue;
            last = code;
            if (code < 0) ds_atomic_or(&lb[DS_FLAG_WORD], 1u);
            else ds_atomic_or(&lb[code >> 5], 1u << (code & 31));
        }
    }
    __syncthreads();
    if (tid < DLKA_DSTATS_LABEL_WORDS && lb[tid]) ds_atomic_or(bitmap + tid, lb[tid]);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------
static_assert((DLKA_DSTATS_LABEL_MAX - DLKA_DSTATS_LABEL_MIN) / 32 + 1 == DS_FLAG_WORD, "one bit per label value, then the flag word");
static_assert(sizeof(DsRanks) <= 256, "the ranks travel in the kernel arguments");

static int ds_check(const dlka_dstats_desc *d, long &cells)
{
    if (!d) return DLKA_ERR_NULL;
    if (d->rank < 2 || d->rank > 3) return DLKA_ERR_SHAPE;
    if (d->C < 1 || d->step < 1) return DLKA_ERR_SHAPE;
    if (d->label_dtype != DLKA_DSTATS_F32 && d->label_dtype != DLKA_DSTATS_I32) return DLKA_ERR_DTYPE;
    if (d->C > DLKA_PREP_C_MAX || d->step > 0x7fffffffL) return DLKA_ERR_UNSUPPORTED;
    cells = 1;                                    // (below 2^31: ranks and offsets are 32-bit)
    const int rc = check_extents(3, {{d->ext, 0x7fffffffL, nullptr, &cells, nullptr}});
    if (rc != DLKA_OK) return rc;
    if (d->rank == 2 && d->ext[0] != 1) return DLKA_ERR_SHAPE;
    return DLKA_OK;
}

static long ds_tiles(long cells) { return cdivl(cells, DS_TILE); }
static unsigned ds_tile_grid(long cells) { return (unsigned)cdivl(ds_tiles(cells), DS_WAVES); }
static int ds_blocks(long n)
{
    const long b = cdivl(n, DS_CHUNK);
    return (int)(b < 1 ? 1 : b > DS_BLOCKS_MAX ? DS_BLOCKS_MAX : b);
}

}  // namespace dlka

using namespace dlka;

extern "C" size_t dlka_dstats_fg_workspace_bytes(const dlka_dstats_desc *d)
{
    long cells;
    if (ds_check(d, cells) != DLKA_OK) return 0;
    return (size_t)ds_tiles(cells) * sizeof(int);
}

extern "C" int dlka_dstats_fg_count(const void *seg, const dlka_dstats_desc *d, void *workspace, size_t workspace_bytes, int64_t *count,
                                    void *stream)
{
    long N;
    const int rc = ds_check(d, N);
    if (rc != DLKA_OK) return rc;
    if (!seg || !count) return DLKA_ERR_NULL;
    if (!workspace || workspace_bytes < dlka_dstats_fg_workspace_bytes(d) || ((uintptr_t)workspace & 3) != 0) return DLKA_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int *counts = (int *)workspace;
    const long T = ds_tiles(N);
    g_dstats_launches.add(2);
    if (d->label_dtype == DLKA_DSTATS_F32)
        DLKA_LAUNCH(dlka_dstats_fg_count_kernel<float>, dim3(ds_tile_grid(N)), dim3(DS_THREADS), 0, st, (const float *)seg, counts, N, T);
    else
        DLKA_LAUNCH(dlka_dstats_fg_count_kernel<int>, dim3(ds_tile_grid(N)), dim3(DS_THREADS), 0, st, (const int *)seg, counts, N, T);
    DLKA_CHECK_LAUNCH();
    DLKA_LAUNCH(dlka_dstats_fg_scan_kernel, dim3(1), dim3(DS_THREADS), 0, st, counts, (long long *)count, T);
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}

extern "C" int dlka_dstats_fg_sample(const float *data, const void *seg, const dlka_dstats_desc *d, const void *offsets, size_t offsets_bytes,
                                     int64_t out_count, float *out, int64_t out_stride, int64_t out_offset, void *stream)
{
    long N;
    const int rc = ds_check(d, N);
    if (rc != DLKA_OK) return rc;
    if (!data || !seg || !out) return DLKA_ERR_NULL;
    if (out_count < 1 || out_offset < 0 || out_count > cdivl(N, d->step) || out_offset + out_count > out_stride) return DLKA_ERR_SHAPE;
    if (!offsets || offsets_bytes < dlka_dstats_fg_workspace_bytes(d) || ((uintptr_t)offsets & 3) != 0) return DLKA_ERR_WORKSPACE;
    DsSampleArgs a = {};
    a.C = d->C; a.step = (unsigned)d->step; a.N = N; a.T = ds_tiles(N);
    a.out_count = out_count; a.out_stride = out_stride; a.out_offset = out_offset;
    hipStream_t st = (hipStream_t)stream;
    g_dstats_launches.add();
    if (d->label_dtype == DLKA_DSTATS_F32)
        DLKA_LAUNCH(dlka_dstats_fg_sample_kernel<float>, dim3(ds_tile_grid(N)), dim3(DS_THREADS), 0, st, data, (const float *)seg,
                    (const int *)offsets, out, a);
    else
        DLKA_LAUNCH(dlka_dstats_fg_sample_kernel<int>, dim3(ds_tile_grid(N)), dim3(DS_THREADS), 0, st, data, (const int *)seg,
                    (const int *)offsets, out, a);
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}

static int ds_check_count(int64_t n)
{
    if (n < 1) return DLKA_ERR_SHAPE;
    if (n >= (1LL << 32)) return DLKA_ERR_UNSUPPORTED;
    return DLKA_OK;
}

extern "C" size_t dlka_dstats_moments_workspace_bytes(int64_t n)
{
    if (ds_check_count(n) != DLKA_OK) return 0;
    return (size_t)ds_blocks(n) * 2 * sizeof(double);
}

extern "C" int dlka_dstats_moments(const float *x, int64_t n, void *workspace, size_t workspace_bytes, double *result, void *stream)
{
    const int rc = ds_check_count(n);
    if (rc != DLKA_OK) return rc;
    if (!x || !result) return DLKA_ERR_NULL;
    if (!workspace || workspace_bytes < dlka_dstats_moments_workspace_bytes(n) || ((uintptr_t)workspace & 7) != 0) return DLKA_ERR_WORKSPACE;
    const int nblk = ds_blocks(n);
    hipStream_t st = (hipStream_t)stream;
    double *partials = (double *)workspace;
    g_dstats_launches.add(4);
    for (int pass = 0; pass < 2; ++pass) {
        DLKA_LAUNCH(dlka_dstats_moments_kernel, dim3((unsigned)nblk), dim3(DS_THREADS), 0, st, x, (const double *)result, partials, (long)n, pass);
        DLKA_CHECK_LAUNCH();
        DLKA_LAUNCH(dlka_dstats_moments_finish_kernel, dim3(1), dim3(64), 0, st, (const double *)partials, result, (long)n, nblk, pass);
        DLKA_CHECK_LAUNCH();
    }
    return DLKA_OK;
}

extern "C" size_t dlka_dstats_select_workspace_bytes(void) { return sizeof(DsSelState); }

extern "C" int dlka_dstats_select(const float *x, int64_t n, const int64_t *ranks, int32_t n_ranks, void *workspace, size_t workspace_bytes,
                                  float *values, int64_t *nan_count, void *stream)
{
    const int rc = ds_check_count(n);
    if (rc != DLKA_OK) return rc;
    if (!x || !ranks || !values) return DLKA_ERR_NULL;
    if (n_ranks < 1) return DLKA_ERR_SHAPE;
    if (n_ranks > DLKA_DSTATS_RANKS_MAX) return DLKA_ERR_UNSUPPORTED;
    DsRanks r = {};
    r.n = n_ranks;
    for (int j = 0; j < n_ranks; ++j) {
        if (ranks[j] < 0 || ranks[j] >= n) return DLKA_ERR_SHAPE;
        r.r[j] = (ds_u64)ranks[j];
    }
    if (!workspace || workspace_bytes < sizeof(DsSelState) || ((uintptr_t)workspace & 7) != 0) return DLKA_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    DsSelState *state = (DsSelState *)workspace;
    const int nblk = ds_blocks(n);
    g_dstats_launches.add(9);
    DLKA_LAUNCH(dlka_dstats_select_init_kernel, dim3(1), dim3(DS_THREADS), 0, st, state, r);
    DLKA_CHECK_LAUNCH();
    for (int pass = 0; pass < 4; ++pass) {
        DLKA_LAUNCH(dlka_dstats_select_hist_kernel, dim3((unsigned)nblk), dim3(DS_THREADS), 0, st, x, (long)n, state, pass);
        DLKA_CHECK_LAUNCH();
        DLKA_LAUNCH(dlka_dstats_select_pick_kernel, dim3(1), dim3(DS_THREADS), 0, st, state, (int)n_ranks, pass, values, (long long *)nan_count);
        DLKA_CHECK_LAUNCH();
    }
    return DLKA_OK;
}

extern "C" int dlka_dstats_unique_labels(const void *seg, const dlka_dstats_desc *d, uint32_t *bitmap, void *stream)
{
    long N;
    const int rc = ds_check(d, N);
    if (rc != DLKA_OK) return rc;
    if (!seg || !bitmap) return DLKA_ERR_NULL;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(bitmap, 0, DLKA_DSTATS_LABEL_WORDS * sizeof(uint32_t), st) != hipSuccess) return DLKA_ERR_LAUNCH;
    const long want = cdivl(N, (long)DS_THREADS * DS_PER);
    const unsigned grid = (unsigned)(want > DS_BLOCKS_MAX ? DS_BLOCKS_MAX : want);
    g_dstats_launches.add();
    if (d->label_dtype == DLKA_DSTATS_F32)
        DLKA_LAUNCH(dlka_dstats_labels_kernel<float>, dim3(grid), dim3(DS_THREADS), 0, st, (const float *)seg, N, (unsigned *)bitmap);
    else
        DLKA_LAUNCH(dlka_dstats_labels_kernel<int>, dim3(grid), dim3(DS_THREADS), 0, st, (const int *)seg, N, (unsigned *)bitmap);
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}
