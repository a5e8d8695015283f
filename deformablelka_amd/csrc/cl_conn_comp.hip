// Connected components of label maps and nnU-Net's "keep the largest component" filter (include/dlka.h: dlka_cc_*): what
// remove_all_but_the_largest_connected_component (3D/d_lka_former/postprocessing/connected_components.py:48-105) computes on one host core with
// one scipy.ndimage.label per class or region and one full-volume comparison per object.
//
// A pass works on one map of extents (ed, eh, ew) and up to DLKA_CC_K_MAX ENTRIES, each a set of class ids (pairwise disjoint): a cell belongs to
// at most one entry, and two neighbouring cells (scipy's generate_binary_structure(rank, connectivity); outside the array is background) are
// connected iff they belong to the same entry.  No mask is materialised: one byte per cell holds the entry.
//
// Union-find over cells in a REVERSED index space i' = N - 1 - i: parent[i'] >= i' always, a root has parent[i'] == i', so the root of a
// component is its largest i', i.e. its first cell in raster order.  The only write of the union step is old = atomicMax(&parent[a], b), a < b.
//
//   local     a workgroup labels a tile of CC_TILE cells in LDS (the same union-find on local reversed indices), then every cell stores the
//             GLOBAL reversed index of its tile-local root, its entry byte, and a zero size.
//   merge     one lane per cell: for every neighbour "behind" it in raster order that lies in ANOTHER tile and has the same entry, unite in
//             global memory.
//   flatten   every cell follows its chain to the root (reads only) and stores it in the component map; sizes: runs of equal roots among the
//             64 lanes of a wave (__shfl_up, __ballot) add their length to the root's counter with one integer atomicAdd; roots per block.
//   scan      one workgroup: exclusive scan of the per-block root counts; the total is the number of components.
//   rank      every root gets 1 + the number of roots before it in raster order (scipy's numbering, which follows the first cell) and raises
//             its entry's largest size with atomicMax.
//   output    component numbers, the filtered map, and per entry the largest removed size (atomicMax).
//   table     (own call) sizes and owning entries by component number.
//
// Forward progress: no grid barrier, no lock, no loop in which a lane waits for another lane's write.  find() walks parent links, which strictly
// increase; unite() retries with (old, b) when its atomicMax met a cell that had been hooked in the meantime, and min(a, b) strictly increases
// from one attempt to the next: both loops end after fewer than N steps whatever the other lanes do, and a stale read (an older parent) only
// makes a walk start lower.  Why a lost race loses nothing: atomicMax leaves parent[a] = max(old, b); the link a -> old that it may have replaced
// by a -> b is re-established by uniting (old, b), which the same lane does next.
//
// Determinism: the partition is the transitive closure of the neighbour relation, whatever order the atomics land in; the root of a component is
// its minimum raster index; sizes and root counts are integer sums; the per-entry maxima are maxima.  The tree SHAPES differ between runs, and
// nothing derived from them is kept: parent[] is workspace.  Two runs give the same bits in every output.
#include "cl_pipeline.h"

DLKA_LAUNCH_COUNTER(g_cc_launches, dlka_cc_launch_count)

namespace dlka {

#define CC_THREADS 256
#define CC_PER 8                          // cells per lane in the tile and block passes
#define CC_TILE (CC_THREADS * CC_PER)     // 2048 cells: a tile of the local pass (4 x 8 x 64, 1 x 32 x 64 or 1 x 1 x 2048), a block of flatten / rank
#define CC_BG 0xff                        // entry byte of a background cell
#define CC_NONE 0xffffffffu               // "no root" in the component map between flatten and output (reversed indices are < 2^31)

struct CcArgs {
    int ext[3];
    int lw, lh, ld;                       // log2 of the tile's extents along w, h, d
    int conn, K, mask_mode, n_ids, has_min;
    unsigned N;
    long id[DLKA_CC_IDS_MAX];
    unsigned char ent_of[DLKA_CC_IDS_MAX];
    unsigned thr[DLKA_CC_K_MAX];          // has_min: a component of fewer cells than this (and not the largest) is removed
};

// summary[DLKA_CC_SUMMARY]: [0] components, [1 + e] largest size of entry e, [1 + K_MAX + e] largest removed size of entry e
#define CC_SUM_MAX(e) (1 + (e))
#define CC_SUM_REM(e) (1 + DLKA_CC_K_MAX + (e))

__device__ __forceinline__ unsigned cc_load(const unsigned *p)
{
#if defined(HIPEMU)
    return __atomic_load_n(p, __ATOMIC_RELAXED);
#else
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (another XCD's atomicMax is not seen through L1 / the own L2)
#endif
}

__device__ __forceinline__ unsigned cc_find(const unsigned *parent, unsigned x)
{
    for (;;) {
        const unsigned p = cc_load(parent + x);
        if (p <= x) return x;             // p == x: a root (p < x never occurs; it ends the walk all the same)
        x = p;
    }
}

__device__ __forceinline__ void cc_unite(unsigned *parent, unsigned a, unsigned b)
{
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a > b) { const unsigned t = a; a = b; b = t; }
        const unsigned old = atomicMax(parent + a, b);
        if (old == a) return;             // a was a root and now hangs below b
        a = old;                          // a had been hooked below `old` meanwhile: parent[a] = max(old, b) now, (old, b) is still to unite
    }
}

template <typename L> __device__ __forceinline__ int cc_entry(const CcArgs &a, L v)
{
    const long x = (long)v;
    if (a.mask_mode) return x != 0 ? 0 : CC_BG;
    int e = CC_BG;
    for (int j = 0; j < a.n_ids; ++j)
        if (a.id[j] == x) e = a.ent_of[j];
    return e;
}

// is (dz, dy, dx) a neighbour offset of this connectivity that lies BEHIND the cell in raster order?
__device__ __forceinline__ bool cc_behind(int conn, int dz, int dy, int dx)
{
    const int l1 = (dz != 0) + (dy != 0) + (dx != 0);
    if (l1 == 0 || l1 > conn) return false;
    return dz < 0 || (dz == 0 && (dy < 0 || (dy == 0 && dx < 0)));
}

// one workgroup per tile; local cell l = (lz, ly, lx), lane tid owns l = tid + 256 j
template <typename L>
__global__ __launch_bounds__(CC_THREADS) void dlka_cc_local_kernel(const CcArgs a, const L *__restrict__ img, unsigned *__restrict__ parent,
                                                                   unsigned char *__restrict__ ent, int *__restrict__ cnt)
{
    __shared__ unsigned lp[CC_TILE];
    __shared__ unsigned char le[CC_TILE];
    const int tid = threadIdx.x;
    const int ed = a.ext[0], eh = a.ext[1], ew = a.ext[2];
    const int tw = 1 << a.lw, th = 1 << a.lh;
    const int ntw = (ew + tw - 1) >> a.lw, nth = (eh + th - 1) >> a.lh;
    const int tx = (int)(blockIdx.x % ntw), ty = (int)((blockIdx.x / ntw) % nth), tz = (int)(blockIdx.x / ((unsigned)ntw * nth));
    const int w0 = tx << a.lw, h0 = ty << a.lh, d0 = tz << a.ld;
#pragma unroll
    for (int j = 0; j < CC_PER; ++j) {
        const int l = tid + CC_THREADS * j;
        const int w = w0 + (l & (tw - 1)), h = h0 + ((l >> a.lw) & (th - 1)), d = d0 + (l >> (a.lw + a.lh));
        int e = CC_BG;
        if (d < ed && h < eh && w < ew) e = cc_entry(a, img[((long)d * eh + h) * ew + w]);
        le[l] = (unsigned char)e;
        lp[CC_TILE - 1 - l] = (unsigned)(CC_TILE - 1 - l);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CC_PER; ++j) {
        const int l = tid + CC_THREADS * j;
        const int e = le[l];
        if (e == CC_BG) continue;
        const int lx = l & (tw - 1), ly = (l >> a.lw) & (th - 1), lz = l >> (a.lw + a.lh);
        for (int dz = -1; dz <= 0; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!cc_behind(a.conn, dz, dy, dx)) continue;
                    const int z = lz + dz, y = ly + dy, x = lx + dx;
                    if (z < 0 || y < 0 || y >= th || x < 0 || x >= tw) continue;     // another tile's cell: the merge pass
                    const int nl = (((z << a.lh) + y) << a.lw) + x;
                    if (le[nl] == e) cc_unite(lp, (unsigned)(CC_TILE - 1 - l), (unsigned)(CC_TILE - 1 - nl));
                }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CC_PER; ++j) {
        const int l = tid + CC_THREADS * j;
        const int w = w0 + (l & (tw - 1)), h = h0 + ((l >> a.lw) & (th - 1)), d = d0 + (l >> (a.lw + a.lh));
        if (d >= ed || h >= eh || w >= ew) continue;
        const unsigned i = (unsigned)(((long)d * eh + h) * ew + w);
        const int r = CC_TILE - 1 - (int)cc_find(lp, (unsigned)(CC_TILE - 1 - l));   // the first cell of the local component: in the array
        const int rw = w0 + (r & (tw - 1)), rh = h0 + ((r >> a.lw) & (th - 1)), rd = d0 + (r >> (a.lw + a.lh));
        parent[a.N - 1 - i] = a.N - 1 - (unsigned)(((long)rd * eh + rh) * ew + rw);
        ent[i] = le[l];
        cnt[i] = 0;
    }
}

// one lane per cell
__global__ __launch_bounds__(CC_THREADS) void dlka_cc_merge_kernel(const CcArgs a, unsigned *__restrict__ parent, const unsigned char *__restrict__ ent)
{
    const unsigned i = blockIdx.x * (unsigned)CC_THREADS + threadIdx.x;
    if (i >= a.N) return;
    const int e = ent[i];
    if (e == CC_BG) return;
    const int eh = a.ext[1], ew = a.ext[2];
    const int w = (int)(i % (unsigned)ew), h = (int)((i / (unsigned)ew) % (unsigned)eh), d = (int)(i / ((unsigned)ew * (unsigned)eh));
    const int tw = 1 << a.lw, th = 1 << a.lh, td = 1 << a.ld;
    const int lx = w & (tw - 1), ly = h & (th - 1), lz = d & (td - 1);
    for (int dz = -1; dz <= 0; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if (!cc_behind(a.conn, dz, dy, dx)) continue;
                if (lz + dz >= 0 && ly + dy >= 0 && ly + dy < th && lx + dx >= 0 && lx + dx < tw) continue;   // same tile: done in LDS
                const int z = d + dz, y = h + dy, x = w + dx;
                if (z < 0 || y < 0 || y >= eh || x < 0 || x >= ew) continue;                                   // outside the array: background
                const unsigned n = (unsigned)(((long)z * eh + y) * ew + x);
                if (ent[n] == e) cc_unite(parent, a.N - 1 - i, a.N - 1 - n);
            }
}

// block b owns cells [b CC_TILE, (b + 1) CC_TILE); lane tid the cells b CC_TILE + 256 j + tid.  root[] is the component map's storage.
__global__ __launch_bounds__(CC_THREADS) void dlka_cc_flatten_kernel(const CcArgs a, const unsigned *__restrict__ parent, const unsigned char *__restrict__ ent,
                                                                     unsigned *__restrict__ root, int *__restrict__ cnt, int *__restrict__ blocksum)
{
    __shared__ int wsum[CC_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    int roots = 0;
    for (int j = 0; j < CC_PER; ++j) {    // (uniform trip count: every lane takes part in the shuffle and the ballots)
        const unsigned long i = (unsigned long)blockIdx.x * CC_TILE + (unsigned)(CC_THREADS * j + tid);
        unsigned r = CC_NONE;
        if (i < a.N && ent[i] != CC_BG) r = cc_find(parent, a.N - 1 - (unsigned)i);
        if (i < a.N) root[i] = r;
        const unsigned prev = __shfl_up(r, 1);
        const bool head = lane == 0 || prev != r;
        const unsigned long long heads = __ballot(head ? 1 : 0);
        if (head && r != CC_NONE) {
            const unsigned long long rest = lane == 63 ? 0ull : heads >> (lane + 1);
            atomicAdd(cnt + (a.N - 1 - r), rest ? __builtin_ctzll(rest) + 1 : 64 - lane);
        }
        roots += __popcll(__ballot((i < a.N && r == a.N - 1 - (unsigned)i) ? 1 : 0));
    }
    if (lane == 0) wsum[tid >> 6] = roots;
    __syncthreads();
    if (tid == 0) blocksum[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// one workgroup: blocksum[] becomes its exclusive scan; summary[0] = the total
__global__ __launch_bounds__(CC_THREADS) void dlka_cc_scan_kernel(int nb, int *__restrict__ blocksum, unsigned *__restrict__ summary)
{
    __shared__ int s[CC_THREADS];
    const int tid = threadIdx.x;
    int carry = 0;
    for (int base = 0; base < nb; base += CC_THREADS) {
        const int v = base + tid < nb ? blocksum[base + tid] : 0;
        s[tid] = v;
        __syncthreads();
        for (int off = 1; off < CC_THREADS; off <<= 1) {
            const int u = tid >= off ? s[tid - off] : 0;
            __syncthreads();
            s[tid] += u;
            __syncthreads();
        }
        if (base + tid < nb) blocksum[base + tid] = carry + s[tid] - v;
        carry += s[CC_THREADS - 1];
        __syncthreads();
    }
    if (tid == 0) summary[0] = (unsigned)carry;
}

// rank[i] (the storage of parent[], no longer read) = number of roots before root i in raster order
__global__ __launch_bounds__(CC_THREADS) void dlka_cc_rank_kernel(const CcArgs a, const unsigned *__restrict__ root, const unsigned char *__restrict__ ent,
                                                                  const int *__restrict__ cnt, const int *__restrict__ blocksum,
                                                                  unsigned *__restrict__ rank, unsigned *__restrict__ summary)
{
    __shared__ int wsum[CC_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int run = blocksum[blockIdx.x];
    for (int j = 0; j < CC_PER; ++j) {
        const unsigned long i = (unsigned long)blockIdx.x * CC_TILE + (unsigned)(CC_THREADS * j + tid);
        const bool flag = i < a.N && root[i] == a.N - 1 - (unsigned)i;
        const unsigned long long m = __ballot(flag ? 1 : 0);
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int before = run;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        if (flag) {
            rank[i] = (unsigned)(before + __popcll(m & ((1ull << lane) - 1ull)));
            atomicMax(summary + CC_SUM_MAX(ent[i]), (unsigned)cnt[i]);
        }
        run += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
}

// labels (in: reversed root index or CC_NONE; out: component number, 0 = background), the filtered map (optional), the largest removed sizes
template <typename L>
__global__ __launch_bounds__(CC_THREADS) void dlka_cc_output_kernel(const CcArgs a, const L *__restrict__ img, const unsigned char *__restrict__ ent,
                                                                    const int *__restrict__ cnt, const unsigned *__restrict__ rank,
                                                                    unsigned *__restrict__ labels, L *__restrict__ filtered, unsigned *__restrict__ summary)
{
    const unsigned i = blockIdx.x * (unsigned)CC_THREADS + threadIdx.x;
    if (i >= a.N) return;
    const unsigned r = labels[i];
    if (r == CC_NONE) {
        labels[i] = 0;
        if (filtered) filtered[i] = img[i];
        return;
    }
    const unsigned ri = a.N - 1 - r;
    const int e = ent[i];
    const unsigned c = (unsigned)cnt[ri];
    const bool keep = c == summary[CC_SUM_MAX(e)] || (a.has_min && c >= a.thr[e]);   // every object of the largest size is kept: no tie-break
    labels[i] = rank[ri] + 1u;
    if (filtered) filtered[i] = keep ? img[i] : (L)0;
    if (!keep && ri == i) atomicMax(summary + CC_SUM_REM(e), c);
}

// sizes[r], owner[r] for component number r + 1 < cap + 1; a root is the one cell of its component with a count
__global__ __launch_bounds__(CC_THREADS) void dlka_cc_table_kernel(unsigned N, const unsigned char *__restrict__ ent, const int *__restrict__ cnt,
                                                                   const unsigned *__restrict__ rank, long cap, int64_t *__restrict__ sizes,
                                                                   int *__restrict__ owner)
{
    const unsigned i = blockIdx.x * (unsigned)CC_THREADS + threadIdx.x;
    if (i >= N) return;
    const int c = cnt[i];
    if (c <= 0 || ent[i] == CC_BG) return;
    const long r = (long)rank[i];
    if (r >= cap) return;
    sizes[r] = c;
    owner[r] = ent[i];
}

static int cc_check(const dlka_cc_desc *d)
{
    if (!d) return DLKA_ERR_NULL;
    if (d->rank < 1 || d->rank > 3) return DLKA_ERR_SHAPE;
    if (d->connectivity < 1 || d->connectivity > d->rank) return DLKA_ERR_UNSUPPORTED;
    if (!label_bytes(d->label_dtype)) return DLKA_ERR_DTYPE;
    if (d->K < 1 || d->K > DLKA_CC_K_MAX) return DLKA_ERR_UNSUPPORTED;
    long cells = 1;                           // (below 2^31: reversed indices and CC_NONE share 32 bits)
    const int rc = check_extents(3, {{d->ext, 0x7fffffffL, nullptr, &cells, nullptr}});
    if (rc != DLKA_OK) return rc;
    for (int ax = 0; ax < 3 - d->rank; ++ax)
        if (d->ext[ax] != 1) return DLKA_ERR_SHAPE;
    if (d->mask_mode) {
        if (d->K != 1) return DLKA_ERR_UNSUPPORTED;
    } else {
        if (d->n_ids < 1 || d->n_ids > DLKA_CC_IDS_MAX) return DLKA_ERR_UNSUPPORTED;
        for (int j = 0; j < d->n_ids; ++j) {
            if (d->entry_of[j] < 0 || d->entry_of[j] >= d->K) return DLKA_ERR_SHAPE;
            for (int i = 0; i < j; ++i)
                if (d->class_id[i] == d->class_id[j]) return DLKA_ERR_UNSUPPORTED;   // a cell belongs to at most one entry
        }
    }
    if (d->has_min)
        for (int k = 0; k < d->K; ++k)
            if (d->min_count[k] < 0) return DLKA_ERR_SHAPE;
    return DLKA_OK;
}

static CcArgs cc_args(const dlka_cc_desc *d)
{
    CcArgs a = {};
    long N = 1;
    for (int ax = 0; ax < 3; ++ax) { a.ext[ax] = (int)d->ext[ax]; N *= (long)d->ext[ax]; }
    a.N = (unsigned)N;
    // CC_TILE cells per tile: 4 x 8 x 64; a map of depth 1: 1 x 32 x 64; a single line: 1 x 1 x 2048
    if (d->ext[0] == 1 && d->ext[1] == 1) { a.ld = 0; a.lh = 0; a.lw = 11; }
    else if (d->ext[0] == 1) { a.ld = 0; a.lh = 5; a.lw = 6; }
    else { a.ld = 2; a.lh = 3; a.lw = 6; }
    a.conn = d->connectivity; a.K = d->K; a.mask_mode = d->mask_mode ? 1 : 0; a.n_ids = a.mask_mode ? 0 : d->n_ids; a.has_min = d->has_min ? 1 : 0;
    for (int j = 0; j < a.n_ids; ++j) { a.id[j] = (long)d->class_id[j]; a.ent_of[j] = (unsigned char)d->entry_of[j]; }
    for (int k = 0; k < d->K; ++k) a.thr[k] = a.has_min ? (unsigned)(d->min_count[k] > 0x7fffffffL ? 0x7fffffffL : d->min_count[k]) : 0u;
    return a;
}

// workspace: parent / rank [N] u32 | cnt [N] i32 | blocksum [nb] i32 | ent [N] u8
struct CcWs { unsigned *parent; int *cnt; int *blocksum; unsigned char *ent; long nb; size_t bytes; };

static CcWs cc_ws(const CcArgs &a, void *workspace)
{
    CcWs w;
    const size_t N = a.N;
    w.nb = cdivl((long)N, CC_TILE);
    w.parent = (unsigned *)workspace;
    w.cnt = (int *)(w.parent + N);
    w.blocksum = w.cnt + N;
    w.ent = (unsigned char *)(w.blocksum + w.nb);
    w.bytes = 8 * N + 4 * (size_t)w.nb + N;
    return w;
}

template <typename L>
static int cc_run(const CcArgs &a, const CcWs &w, const void *image, unsigned *labels, void *filtered, unsigned *summary, hipStream_t st)
{
    const long ntiles = cdivl(a.ext[2], 1L << a.lw) * cdivl(a.ext[1], 1L << a.lh) * cdivl(a.ext[0], 1L << a.ld);
    const unsigned cellgrid = (unsigned)cdivl((long)a.N, CC_THREADS);
    if (hipMemsetAsync(summary, 0, DLKA_CC_SUMMARY * sizeof(unsigned), st) != hipSuccess) return DLKA_ERR_LAUNCH;
    g_cc_launches.add(6);
    auto local = dlka_cc_local_kernel<L>;
    auto output = dlka_cc_output_kernel<L>;
    DLKA_LAUNCH(local, dim3((unsigned)ntiles), dim3(CC_THREADS), 0, st, a, (const L *)image, w.parent, w.ent, w.cnt);
    DLKA_CHECK_LAUNCH();
    DLKA_LAUNCH(dlka_cc_merge_kernel, dim3(cellgrid), dim3(CC_THREADS), 0, st, a, w.parent, (const unsigned char *)w.ent);
    DLKA_CHECK_LAUNCH();
    DLKA_LAUNCH(dlka_cc_flatten_kernel, dim3((unsigned)w.nb), dim3(CC_THREADS), 0, st, a, (const unsigned *)w.parent, (const unsigned char *)w.ent, labels,
                w.cnt, w.blocksum);
    DLKA_CHECK_LAUNCH();
    DLKA_LAUNCH(dlka_cc_scan_kernel, dim3(1), dim3(CC_THREADS), 0, st, (int)w.nb, w.blocksum, summary);
    DLKA_CHECK_LAUNCH();
    DLKA_LAUNCH(dlka_cc_rank_kernel, dim3((unsigned)w.nb), dim3(CC_THREADS), 0, st, a, (const unsigned *)labels, (const unsigned char *)w.ent,
                (const int *)w.cnt, (const int *)w.blocksum, w.parent, summary);
    DLKA_CHECK_LAUNCH();
    DLKA_LAUNCH(output, dim3(cellgrid), dim3(CC_THREADS), 0, st, a, (const L *)image, (const unsigned char *)w.ent, (const int *)w.cnt,
                (const unsigned *)w.parent, labels, (L *)filtered, summary);
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}

}  // namespace dlka

using namespace dlka;

extern "C" size_t dlka_cc_workspace_bytes(const dlka_cc_desc *d)
{
    if (cc_check(d) != DLKA_OK) return 0;
    return cc_ws(cc_args(d), nullptr).bytes;
}

extern "C" int dlka_cc_components(const void *image, const dlka_cc_desc *d, void *workspace, size_t workspace_bytes, int32_t *labels, void *filtered,
                                  int32_t *summary, void *stream)
{
    const int rc = cc_check(d);
    if (rc != DLKA_OK) return rc;
    if (!image || !labels || !summary) return DLKA_ERR_NULL;
    if (filtered == image) return DLKA_ERR_UNSUPPORTED;
    const CcArgs a = cc_args(d);
    const CcWs w = cc_ws(a, workspace);
    if (!workspace || workspace_bytes < w.bytes) return DLKA_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    return dispatch_label(d->label_dtype, [&](auto t) {
        return cc_run<DLKA_T(t)>(a, w, image, (unsigned *)labels, filtered, (unsigned *)summary, st);
    });
}

extern "C" int dlka_cc_component_table(const dlka_cc_desc *d, const void *workspace, size_t workspace_bytes, int64_t capacity, int64_t *sizes,
                                       int32_t *owner, void *stream)
{
    const int rc = cc_check(d);
    if (rc != DLKA_OK) return rc;
    if (capacity < 0) return DLKA_ERR_SHAPE;
    if (capacity == 0) return DLKA_OK;
    if (!sizes || !owner) return DLKA_ERR_NULL;
    const CcArgs a = cc_args(d);
    const CcWs w = cc_ws(a, const_cast<void *>(workspace));
    if (!workspace || workspace_bytes < w.bytes) return DLKA_ERR_WORKSPACE;
    g_cc_launches.add();
    DLKA_LAUNCH(dlka_cc_table_kernel, dim3((unsigned)cdivl((long)a.N, CC_THREADS)), dim3(CC_THREADS), 0, (hipStream_t)stream, a.N,
                (const unsigned char *)w.ent, (const int *)w.cnt, (const unsigned *)w.parent, (long)capacity, sizes, owner);
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}
