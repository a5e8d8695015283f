// Sliding-window prediction with test-time mirroring: the data movement and blending of nnU-Net's
// _internal_predict_3D_3Dconv_tiled (3D/d_lka_former/network_architecture/neural_network.py:292-428) and
// _internal_maybe_mirror_and_pred_3D (:502-560) in three launches per chunk of tiles (include/dlka.h: dlka_tiles_*).
//
//   gather    the network input [T*M][C][pd][ph][pw] of a chunk straight from the UNPADDED volume: padding is a range check
//             (reads outside the volume give the pad value, pad_nd_image(..., 'constant')), a flip is index arithmetic.  A pure
//             copy: bitwise torch.flip of the padded slice.
//   blend     gather form: a thread owns one voxel of the chunk's bounding box and walks the chunk's tiles that cover it, in tile
//             order; per tile r_k = sum_m scale * nonlin(p)[t, m, k, unflipped voxel] in the listed mirror order (:526-557), r_k *= g
//             (:559), score_k += r_k, weight += g (:414-415).  Score and weight of the voxel are read once and written once; no
//             atomics, the addition order is the reference's sequential per-tile order, so the result is bitwise reproducible.
//   finalize probs = score / weight and seg = first-maximum argmax (torch.argmax: NaN wins) over the region the padding slicer keeps
//             (:420-428).
//
// Memory-bound streaming kernels.  Layout for all three: a wave of 64 lanes sweeps one z-row (the contiguous axis), four rows per
// workgroup, so every load and store of a wave covers consecutive words (in reverse lane order where z is flipped: the same lines).
// The per-row index arithmetic (divisions by the extents) is wave-uniform and paid once per row.  Softmax over K runs in registers:
// K is bucketed into a compile-time bound (4 / 8 / 16 / 32) so that the per-class arrays stay in VGPRs.
#include <math.h>

#include "cl_pipeline.h"

DLKA_LAUNCH_COUNTER(g_tiles_launches, dlka_tiles_launch_count)

namespace dlka {

struct TilesArgs {
    int T, M, C, K;
    int pd, ph, pw;
    int X, Y, Z;           // gather: unpadded volume; finalize: kept region
    int lx, ly, lz;        // low-side padding
    int Xp, Yp, Zp;        // padded extents (blend, finalize)
    int bx0, by0, bz0, bxn, byn, bzn;   // blend: the chunk's bounding box
    float pad_value, scale;
    int ox[DLKA_TILES_MAX_T], oy[DLKA_TILES_MAX_T], oz[DLKA_TILES_MAX_T];
    int mask[8];
};

#define TILES_ROWS 4   // z-rows (waves) per workgroup
static long tiles_blocks(long rows) { return cdivl(rows, TILES_ROWS); }

__global__ __launch_bounds__(64 * TILES_ROWS) void dlka_tiles_gather_kernel(const TilesArgs a, const float *__restrict__ x,
                                                                          float *__restrict__ out, long nrows)
{
    const long row = (long)blockIdx.x * TILES_ROWS + threadIdx.y;   // (b, c, i, j)
    if (row >= nrows) return;
    long r = row;
    const int j = (int)(r % a.ph); r /= a.ph;
    const int i = (int)(r % a.pd); r /= a.pd;
    const int c = (int)(r % a.C); r /= a.C;
    const int m = (int)(r % a.M);
    const int t = (int)(r / a.M);
    const int mk = a.mask[m];
    const int xi = a.ox[t] + ((mk & 1) ? a.pd - 1 - i : i) - a.lx;
    const int yi = a.oy[t] + ((mk & 2) ? a.ph - 1 - j : j) - a.ly;
    const bool row_in = xi >= 0 && xi < a.X && yi >= 0 && yi < a.Y;
    const float *src = x + (((long)c * a.X + (row_in ? xi : 0)) * a.Y + (row_in ? yi : 0)) * a.Z;
    float *dst = out + row * a.pw;
    const int zb = a.oz[t] - a.lz;
    for (int k = threadIdx.x; k < a.pw; k += 64) {
        const int zi = zb + ((mk & 4) ? a.pw - 1 - k : k);
        dst[k] = (row_in && zi >= 0 && zi < a.Z) ? src[zi] : a.pad_value;
    }
}

template <int KB, int NL>
__device__ __forceinline__ void tiles_nonlin(float (&l)[KB], int K)
{
    if (NL == DLKA_TILES_SOFTMAX) {   // torch.softmax(x, 1): exp(x - max) / sum
        float mx = l[0];
#pragma unroll
        for (int k = 1; k < KB; ++k)
            if (k < K) mx = fmaxf(mx, l[k]);
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < KB; ++k)
            if (k < K) { l[k] = expf(l[k] - mx); s += l[k]; }
#pragma unroll
        for (int k = 0; k < KB; ++k)
            if (k < K) l[k] = l[k] / s;
    } else if (NL == DLKA_TILES_SIGMOID) {
#pragma unroll
        for (int k = 0; k < KB; ++k)
            if (k < K) l[k] = 1.f / (1.f + expf(-l[k]));
    }
}

template <typename T, int KB, int NL>
__global__ __launch_bounds__(64 * TILES_ROWS) void dlka_tiles_blend_kernel(const TilesArgs a, const T *__restrict__ logits,
                                                                         const float *__restrict__ gauss, float *__restrict__ score,
                                                                         float *__restrict__ weight)
{
    // The reference rounds every product and sum on its own (r * g, then score + that): no contraction into FMAs here.
#pragma clang fp contract(off)
    const int row = blockIdx.x * TILES_ROWS + threadIdx.y;   // (x, y) of the bounding box
    if (row >= a.bxn * a.byn) return;
    const int vx = a.bx0 + row / a.byn, vy = a.by0 + row % a.byn;
    const long P = (long)a.pd * a.ph * a.pw;
    const long V = (long)a.Xp * a.Yp * a.Zp;
    for (int zz = threadIdx.x; zz < a.bzn; zz += 64) {
        const int vz = a.bz0 + zz;
        const long vo = ((long)vx * a.Yp + vy) * a.Zp + vz;
        float acc[KB] = {};
        float wacc = 0.f;
        bool loaded = false;
        for (int t = 0; t < a.T; ++t) {
            const int i = vx - a.ox[t], j = vy - a.oy[t], k = vz - a.oz[t];
            if ((unsigned)i >= (unsigned)a.pd || (unsigned)j >= (unsigned)a.ph || (unsigned)k >= (unsigned)a.pw) continue;
            if (!loaded) {
#pragma unroll
                for (int c = 0; c < KB; ++c)
                    if (c < a.K) acc[c] = score[c * V + vo];
                wacc = weight[vo];
                loaded = true;
            }
            float r[KB];
#pragma unroll
            for (int c = 0; c < KB; ++c) r[c] = 0.f;
            for (int m = 0; m < a.M; ++m) {
                const int mk = a.mask[m];
                const int ii = (mk & 1) ? a.pd - 1 - i : i, jj = (mk & 2) ? a.ph - 1 - j : j, kk = (mk & 4) ? a.pw - 1 - k : k;
                const T *p = logits + (long)(t * a.M + m) * a.K * P + ((long)ii * a.ph + jj) * a.pw + kk;
                float l[KB];
#pragma unroll
                for (int c = 0; c < KB; ++c) l[c] = (c < a.K) ? ldf(p + c * P) : 0.f;
                tiles_nonlin<KB, NL>(l, a.K);
#pragma unroll
                for (int c = 0; c < KB; ++c)
                    if (c < a.K) r[c] = r[c] + a.scale * l[c];
            }
            const float g = gauss ? gauss[((long)i * a.ph + j) * a.pw + k] : 1.f;
#pragma unroll
            for (int c = 0; c < KB; ++c)
                if (c < a.K) acc[c] = acc[c] + r[c] * g;
            wacc = wacc + g;
        }
        if (loaded) {
#pragma unroll
            for (int c = 0; c < KB; ++c)
                if (c < a.K) score[c * V + vo] = acc[c];
            weight[vo] = wacc;
        }
    }
}

__global__ __launch_bounds__(64 * TILES_ROWS) void dlka_tiles_finalize_kernel(const TilesArgs a, const float *__restrict__ score,
                                                                            const float *__restrict__ weight, float *__restrict__ probs,
                                                                            int64_t *__restrict__ seg)
{
    const long row = (long)blockIdx.x * TILES_ROWS + threadIdx.y;   // (x, y) of the kept region
    if (row >= (long)a.X * a.Y) return;
    const int x = (int)(row / a.Y), y = (int)(row % a.Y);
    const long V = (long)a.Xp * a.Yp * a.Zp, N = (long)a.X * a.Y * a.Z;
    const long src = ((long)(x + a.lx) * a.Yp + (y + a.ly)) * a.Zp + a.lz;
    for (int z = threadIdx.x; z < a.Z; z += 64) {
        const long o = row * a.Z + z;
        const float w = weight[src + z];
        float best = 0.f;
        int64_t idx = 0;
        for (int c = 0; c < a.K; ++c) {
            const float v = score[c * V + src + z] / w;
            probs[c * N + o] = v;
            if (c == 0 || (!isnan(best) && (isnan(v) || v > best))) { best = v; idx = c; }
        }
        seg[o] = idx;
    }
}

template <typename T, int KB>
static void launch_blend_nl(const TilesArgs &a, int nonlin, const T *logits, const float *g, float *score, float *weight, unsigned blocks,
                            hipStream_t st)
{
    const dim3 block(64, TILES_ROWS);
    if (nonlin == DLKA_TILES_SOFTMAX) { auto k = dlka_tiles_blend_kernel<T, KB, DLKA_TILES_SOFTMAX>; DLKA_LAUNCH(k, dim3(blocks), block, 0, st, a, logits, g, score, weight); }
    else if (nonlin == DLKA_TILES_SIGMOID) { auto k = dlka_tiles_blend_kernel<T, KB, DLKA_TILES_SIGMOID>; DLKA_LAUNCH(k, dim3(blocks), block, 0, st, a, logits, g, score, weight); }
    else { auto k = dlka_tiles_blend_kernel<T, KB, DLKA_TILES_IDENTITY>; DLKA_LAUNCH(k, dim3(blocks), block, 0, st, a, logits, g, score, weight); }
}

template <typename T>
static void launch_blend_t(const TilesArgs &a, int nonlin, const T *logits, const float *g, float *score, float *weight, unsigned blocks,
                           hipStream_t st)
{
    if (a.K <= 4) launch_blend_nl<T, 4>(a, nonlin, logits, g, score, weight, blocks, st);
    else if (a.K <= 8) launch_blend_nl<T, 8>(a, nonlin, logits, g, score, weight, blocks, st);
    else if (a.K <= 16) launch_blend_nl<T, 16>(a, nonlin, logits, g, score, weight, blocks, st);
    else launch_blend_nl<T, 32>(a, nonlin, logits, g, score, weight, blocks, st);
}

// Shared checks of the chunk description: T tiles, M mirror masks (each in 0..7)
static int tiles_chunk_args(TilesArgs &a, const int *origins, int T, const int *masks, int M, int pd, int ph, int pw)
{
    if (!origins || !masks) return DLKA_ERR_NULL;
    if (T <= 0 || M <= 0 || pd <= 0 || ph <= 0 || pw <= 0) return DLKA_ERR_SHAPE;
    if (T > DLKA_TILES_MAX_T || M > 8) return DLKA_ERR_UNSUPPORTED;
    a.T = T; a.M = M; a.pd = pd; a.ph = ph; a.pw = pw;
    for (int t = 0; t < T; ++t) { a.ox[t] = origins[3 * t]; a.oy[t] = origins[3 * t + 1]; a.oz[t] = origins[3 * t + 2]; }
    for (int m = 0; m < M; ++m) {
        if (masks[m] < 0 || masks[m] > 7) return DLKA_ERR_UNSUPPORTED;
        a.mask[m] = masks[m];
    }
    return DLKA_OK;
}

}  // namespace dlka

using namespace dlka;

extern "C" int dlka_tiles_gather(const float *x, int C, int X, int Y, int Z, const int *origins, int T, const int *masks, int M, int pd, int ph,
                                 int pw, int pad_x, int pad_y, int pad_z, float pad_value, float *out, void *stream)
{
    if (!x || !out) return DLKA_ERR_NULL;
    if (C <= 0 || X <= 0 || Y <= 0 || Z <= 0 || pad_x < 0 || pad_y < 0 || pad_z < 0) return DLKA_ERR_SHAPE;
    TilesArgs a = {};
    const int rc = tiles_chunk_args(a, origins, T, masks, M, pd, ph, pw);
    if (rc != DLKA_OK) return rc;
    a.C = C; a.X = X; a.Y = Y; a.Z = Z; a.lx = pad_x; a.ly = pad_y; a.lz = pad_z; a.pad_value = pad_value;
    const long nrows = (long)T * M * C * pd * ph;
    const long blocks = tiles_blocks(nrows);
    if (blocks > 0x7fffffffL) return DLKA_ERR_UNSUPPORTED;
    g_tiles_launches.add();
    DLKA_LAUNCH(dlka_tiles_gather_kernel, dim3((unsigned)blocks), dim3(64, TILES_ROWS), 0, (hipStream_t)stream, a, x, out, nrows);
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}

extern "C" int dlka_tiles_blend(const void *logits, int dtype, int K, int nonlin, float mirror_scale, const float *gauss, float *score,
                                float *weight, int Xp, int Yp, int Zp, const int *origins, int T, const int *masks, int M, int pd, int ph, int pw,
                                void *stream)
{
    if (!logits || !score || !weight) return DLKA_ERR_NULL;
    return dispatch_storage<ST_F32 | ST_BF16>(dtype, [&](auto tag) -> int {
        if (K <= 0 || Xp <= 0 || Yp <= 0 || Zp <= 0) return DLKA_ERR_SHAPE;
        if (K > DLKA_TILES_K_MAX || nonlin < DLKA_TILES_IDENTITY || nonlin > DLKA_TILES_SIGMOID) return DLKA_ERR_UNSUPPORTED;
        TilesArgs a = {};
        const int rc = tiles_chunk_args(a, origins, T, masks, M, pd, ph, pw);
        if (rc != DLKA_OK) return rc;
        a.K = K; a.Xp = Xp; a.Yp = Yp; a.Zp = Zp; a.scale = mirror_scale;
        int lo[3] = {Xp, Yp, Zp}, hi[3] = {0, 0, 0};
        const int ext[3] = {Xp, Yp, Zp}, p[3] = {pd, ph, pw};
        for (int t = 0; t < T; ++t)
            for (int d = 0; d < 3; ++d) {
                const int o = origins[3 * t + d];
                if (o < 0 || o + p[d] > ext[d]) return DLKA_ERR_SHAPE;   // every tile lies inside the score map
                lo[d] = o < lo[d] ? o : lo[d];
                hi[d] = o + p[d] > hi[d] ? o + p[d] : hi[d];
            }
        a.bx0 = lo[0]; a.by0 = lo[1]; a.bz0 = lo[2];
        a.bxn = hi[0] - lo[0]; a.byn = hi[1] - lo[1]; a.bzn = hi[2] - lo[2];
        g_tiles_launches.add();
        launch_blend_t(a, nonlin, (const DLKA_T(tag) *)logits, gauss, score, weight, (unsigned)tiles_blocks((long)a.bxn * a.byn),
                       (hipStream_t)stream);
        DLKA_CHECK_LAUNCH();
        return DLKA_OK;
    });
}

extern "C" int dlka_tiles_finalize(const float *score, const float *weight, int K, int Xp, int Yp, int Zp, int pad_x, int pad_y, int pad_z, int X,
                                   int Y, int Z, float *probs, int64_t *seg, void *stream)
{
    if (!score || !weight || !probs || !seg) return DLKA_ERR_NULL;
    if (K <= 0 || X <= 0 || Y <= 0 || Z <= 0 || pad_x < 0 || pad_y < 0 || pad_z < 0) return DLKA_ERR_SHAPE;
    if (pad_x + X > Xp || pad_y + Y > Yp || pad_z + Z > Zp) return DLKA_ERR_SHAPE;
    TilesArgs a = {};
    a.K = K; a.Xp = Xp; a.Yp = Yp; a.Zp = Zp; a.lx = pad_x; a.ly = pad_y; a.lz = pad_z; a.X = X; a.Y = Y; a.Z = Z;
    g_tiles_launches.add();
    DLKA_LAUNCH(dlka_tiles_finalize_kernel, dim3((unsigned)tiles_blocks((long)X * Y)), dim3(64, TILES_ROWS), 0, (hipStream_t)stream, a, score, weight, probs, seg);
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}
