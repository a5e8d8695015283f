// The UNETR++ "efficient paired attention" (EPA) on the token tensor, float32, per batch sample b and head h (D = head width, P = proj_size):
//
//   Q, K, Vc, Vs   the four D-wide column groups of qkvv [B][N][4][heads][D] (the Linear's own layout, never transposed or copied)
//   rq_i = 1 / max(|Q[:, i]|, 1e-12), rk_j likewise        column norms over the N tokens (F.normalize after the transpose)
//   A  = softmax_j(Qh^T Kh * temperature[h])  [D][D]       channel branch: x_CA[n][h D + i] = sum_j (A m1)[i][j] Vc[n][j]
//   S  = softmax_p(Qh[n] . Kp * temperature2[h])  [P]      spatial branch:  Y[n][i] = sum_p (S m2)[p] Vp[i][p], stored at the offset the
//                                                          reference's permute(0, 3, 1, 2).reshape(B, N, C) gives it: ((b D + i) heads + h) N + n
//
// Forward: cl_epa_gram_kernel (column sums of squares + the raw Gram Q^T K as per-workgroup partial tiles), cl_epa_finish_kernel (ordered fold,
// norms, the D x D softmax, m1), cl_epa_apply_kernel (Kp / Vp / A of the head in LDS, one token per lane: scores, softmax, both outputs in registers —
// the N x P map never reaches memory).  Backward: cl_epa_bwd_tokens_kernel (S again per token; dQh of the spatial branch into slot 0 of d(qkvv);
// partial tiles of dVp and dKp through an LDS stage), cl_epa_gram_kernel on (dx_CA, Vc), cl_epa_bwd_finish_kernel (folds, the D x D softmax backward,
// dtemperature, the projection terms of the normalisation), cl_epa_bwd_apply_kernel (dQ, dK, dVc rows; slot 3 zeroed: Vs is reached through Vp only).
// No floating-point atomics: every sum over tokens is a per-workgroup partial folded in workgroup order, so two identical calls give the same bits.
#include "dlka_common.h"
#include "dlka_kernels.h"

namespace dlka {

constexpr int EPA_NT = 256;       // threads per workgroup, and tokens per workgroup of the token passes
constexpr int EPA_CHUNK = 256;    // tokens per partial tile of the Gram pass
constexpr int EPA_GT = 32;        // tokens per LDS tile of the Gram pass
constexpr int EPA_ST = 16;        // tokens per LDS stage of the backward token pass
constexpr float EPA_EPS = 1e-12f;

__host__ __device__ constexpr int epa_gram_tile(int D) { return D >= 32 ? D / 16 : 1; }
__host__ __device__ constexpr int epa_gram_floats(int D) { return D * D + 2 * D; }

// part[((b heads + h) nchunk + chunk)][D D + 2 D]: X^T Y over the chunk's tokens, then (SQ) the column sums of squares of X and of Y.
// X / Y: token-major, row stride xs / ys floats, the head's columns start at xo + h D / yo + h D, batch stride xb / yb.
template <int D, bool SQ>
__global__ __launch_bounds__(EPA_NT) void cl_epa_gram_kernel(const float *__restrict__ X, long xb, int xs, int xo, const float *__restrict__ Y, long yb, int ys,
                                                            int yo, float *__restrict__ part, int N, int nchunk)
{
    constexpr int T = epa_gram_tile(D), ND = D / T, PAIRS = ND * ND, S = EPA_NT / PAIRS, GF = epa_gram_floats(D);
    static_assert(PAIRS * S == EPA_NT, "the pairs and their token slices fill the workgroup");
    DLKA_DYN_SMEM(float, sm);   // sX [GT][D], sY [GT][D], red [S][GF]
    float *sX = sm, *sY = sm + EPA_GT * D, *red = sm + 2 * EPA_GT * D;
    const int tid = threadIdx.x, chunk = blockIdx.x, h = blockIdx.y, b = blockIdx.z, heads = gridDim.y;
    const int pj = tid % ND, pi = (tid / ND) % ND, s = tid / PAIRS;
    const float *xp = X + (long)b * xb + xo + h * D, *yp = Y + (long)b * yb + yo + h * D;
    const int n_lo = chunk * EPA_CHUNK, n_hi = n_lo + EPA_CHUNK < N ? n_lo + EPA_CHUNK : N;
    float acc[T][T], sqx[T], sqy[T];
#pragma unroll
    for (int a = 0; a < T; ++a) {
        sqx[a] = sqy[a] = 0.f;
#pragma unroll
        for (int c = 0; c < T; ++c) acc[a][c] = 0.f;
    }
    for (int n0 = n_lo; n0 < n_hi; n0 += EPA_GT) {
        for (int e = tid; e < EPA_GT * D; e += EPA_NT) {
            const int t = e / D, c = e % D, n = n0 + t;
            sX[e] = n < n_hi ? xp[(long)n * xs + c] : 0.f;
            sY[e] = n < n_hi ? yp[(long)n * ys + c] : 0.f;
        }
        __syncthreads();
        for (int t = s; t < EPA_GT; t += S) {
            float xv[T], yv[T];
#pragma unroll
            for (int a = 0; a < T; ++a) { xv[a] = sX[t * D + pi * T + a]; yv[a] = sY[t * D + pj * T + a]; }
#pragma unroll
            for (int a = 0; a < T; ++a) {
                if (SQ) { sqx[a] = fmaf(xv[a], xv[a], sqx[a]); sqy[a] = fmaf(yv[a], yv[a], sqy[a]); }
#pragma unroll
                for (int c = 0; c < T; ++c) acc[a][c] = fmaf(xv[a], yv[c], acc[a][c]);
            }
        }
        __syncthreads();
    }
    float *r = red + s * GF;
#pragma unroll
    for (int a = 0; a < T; ++a) {
#pragma unroll
        for (int c = 0; c < T; ++c) r[(pi * T + a) * D + pj * T + c] = acc[a][c];
        if (pj == 0) r[D * D + pi * T + a] = sqx[a];
        if (pi == 0) r[D * D + D + pj * T + a] = sqy[a];
    }
    __syncthreads();
    float *out = part + ((long)(b * heads + h) * nchunk + chunk) * GF;
    for (int e = tid; e < GF; e += EPA_NT) {
        float v = red[e];
        for (int q = 1; q < S; ++q) v += red[q * GF + e];
        out[e] = v;
    }
}

// One workgroup per (h, b).  Folds the partial tiles in chunk order; nrm[b][5][C] = {1 / max(|q|, eps), 1 / max(|k|, eps), |q| >= eps, |k| >= eps,
// temperature2[h] / max(|q|, eps)}; ghat = the normalised Gram, a_soft = softmax(ghat temperature[h]), a_mask = a_soft m1 (m1 null: not written).
template <int D>
__global__ __launch_bounds__(EPA_NT) void cl_epa_finish_kernel(const float *__restrict__ part, int nchunk, const float *__restrict__ temperature,
                                                              const float *__restrict__ temperature2, const float *__restrict__ m1, float *__restrict__ nrm,
                                                              float *__restrict__ ghat, float *__restrict__ a_soft, float *__restrict__ a_mask, int C)
{
    constexpr int GF = epa_gram_floats(D);
    __shared__ float g[GF];
    __shared__ float rr[2 * D];
    const int tid = threadIdx.x, h = blockIdx.x, b = blockIdx.y, heads = gridDim.x;
    const float *p = part + (long)(b * heads + h) * nchunk * GF;
    for (int e = tid; e < GF; e += EPA_NT) {
        float v = p[e];
        for (int c = 1; c < nchunk; ++c) v += p[(long)c * GF + e];
        g[e] = v;
    }
    __syncthreads();
    if (tid < 2 * D) {
        const float n = sqrtf(g[D * D + tid]);
        const float r = 1.f / fmaxf(n, EPA_EPS);
        rr[tid] = r;
        const int which = tid / D, c = h * D + tid % D;
        float *nb = nrm + (long)b * 5 * C;
        nb[which * C + c] = r;
        nb[(2 + which) * C + c] = n >= EPA_EPS ? 1.f : 0.f;
        if (which == 0) nb[4 * C + c] = r * temperature2[h];
    }
    __syncthreads();
    if (tid < D) {
        const int i = tid;
        const long o = ((long)(b * heads + h) * D + i) * D;
        const float tp = temperature[h];
        float l[D], mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const float gh = g[i * D + j] * rr[i] * rr[D + j];
            ghat[o + j] = gh;
            l[j] = gh * tp;
            mx = fmaxf(mx, l[j]);
        }
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < D; ++j) { l[j] = expf(l[j] - mx); sum += l[j]; }
        const float inv = 1.f / sum;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const float a = l[j] * inv;
            a_soft[o + j] = a;
            if (m1) a_mask[o + j] = a * m1[o + j];
        }
    }
}

// the head's [D][P] projection tile and [D][D] attention tile into LDS
template <int D, int P>
__device__ __forceinline__ void epa_load_head(float *sKp, float *sVp, const float *__restrict__ kp, const float *__restrict__ vp, long o)
{
    for (int e = threadIdx.x; e < D * P; e += EPA_NT) { sKp[e] = kp[o + e]; sVp[e] = vp[o + e]; }
}

// scores of one token against the head's Kp (qh carries temperature2 / |q|), softmax with max subtraction: s[p] on return
template <int D, int P> __device__ __forceinline__ void epa_token_softmax(const float *qh, const float *sKp, float *s)
{
#pragma unroll
    for (int p = 0; p < P; ++p) s[p] = 0.f;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const float q = qh[i];
#pragma unroll
        for (int p = 0; p < P; p += 4) {
            const f32x4 k = *reinterpret_cast<const f32x4 *>(sKp + i * P + p);
            s[p] = fmaf(q, k[0], s[p]); s[p + 1] = fmaf(q, k[1], s[p + 1]); s[p + 2] = fmaf(q, k[2], s[p + 2]); s[p + 3] = fmaf(q, k[3], s[p + 3]);
        }
    }
    float mx = s[0];
#pragma unroll
    for (int p = 1; p < P; ++p) mx = fmaxf(mx, s[p]);
    float sum = 0.f;
#pragma unroll
    for (int p = 0; p < P; ++p) { s[p] = expf(s[p] - mx); sum += s[p]; }
    const float inv = 1.f / sum;
#pragma unroll
    for (int p = 0; p < P; ++p) s[p] *= inv;
}

// mult[p] = m2_scale where the token's mask byte is set, else 0
template <int P> __device__ __forceinline__ void epa_mask_row(const unsigned char *__restrict__ m2, long row, float scale, float *mult)
{
    const unsigned *w = reinterpret_cast<const unsigned *>(m2 + row * P);
#pragma unroll
    for (int p = 0; p < P; p += 4) {
        const unsigned v = w[p / 4];
#pragma unroll
        for (int e = 0; e < 4; ++e) mult[p + e] = ((v >> (8 * e)) & 0xffu) ? scale : 0.f;
    }
}

// grid (ceil(N / 256), heads, B): one token per lane
template <int D, int P, bool MASK>
__global__ __launch_bounds__(EPA_NT) void cl_epa_apply_kernel(const float *__restrict__ qkvv, const float *__restrict__ kp, const float *__restrict__ vp,
                                                             const float *__restrict__ a_mask, const float *__restrict__ nrm,
                                                             const unsigned char *__restrict__ m2, float m2_scale, float *__restrict__ x_sa,
                                                             float *__restrict__ x_ca, int N, int C)
{
    DLKA_DYN_SMEM(float, sm);   // sKp [D][P], sVp [D][P], sA [D][D], sQs [D]
    float *sKp = sm, *sVp = sm + D * P, *sA = sm + 2 * D * P, *sQs = sA + D * D;
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z, heads = gridDim.y;
    epa_load_head<D, P>(sKp, sVp, kp, vp, ((long)b * C + h * D) * P);
    for (int e = tid; e < D * D; e += EPA_NT) sA[e] = a_mask[(long)(b * heads + h) * D * D + e];
    if (tid < D) sQs[tid] = nrm[(long)b * 5 * C + 4 * C + h * D + tid];
    __syncthreads();
    const int n = blockIdx.x * EPA_NT + tid;
    if (n >= N) return;
    const float *row = qkvv + ((long)b * N + n) * 4 * C + h * D;
    float s[P];
    {
        float qh[D];
#pragma unroll
        for (int i = 0; i < D; i += 4) {
            const f32x4 q = *reinterpret_cast<const f32x4 *>(row + i);
            qh[i] = q[0] * sQs[i]; qh[i + 1] = q[1] * sQs[i + 1]; qh[i + 2] = q[2] * sQs[i + 2]; qh[i + 3] = q[3] * sQs[i + 3];
        }
        epa_token_softmax<D, P>(qh, sKp, s);
    }
    if (MASK) {
        float mult[P];
        epa_mask_row<P>(m2, (long)(b * heads + h) * N + n, m2_scale, mult);
#pragma unroll
        for (int p = 0; p < P; ++p) s[p] *= mult[p];
    }
    float *ysa = x_sa + ((long)b * D * heads + h) * N + n;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        float y = 0.f;
#pragma unroll
        for (int p = 0; p < P; p += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(sVp + i * P + p);
            y = fmaf(s[p], v[0], y); y = fmaf(s[p + 1], v[1], y); y = fmaf(s[p + 2], v[2], y); y = fmaf(s[p + 3], v[3], y);
        }
        ysa[(long)i * heads * N] = y;
    }
    float vc[D];
#pragma unroll
    for (int j = 0; j < D; j += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(row + 2 * C + j);
        vc[j] = v[0]; vc[j + 1] = v[1]; vc[j + 2] = v[2]; vc[j + 3] = v[3];
    }
    float *yca = x_ca + ((long)b * N + n) * C + h * D;
#pragma unroll
    for (int i = 0; i < D; i += 4) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float y = 0.f;
#pragma unroll
            for (int j = 0; j < D; ++j) y = fmaf(sA[(i + e) * D + j], vc[j], y);
            o[e] = y;
        }
        *reinterpret_cast<f32x4 *>(yca + i) = o;
    }
}

// Backward, first token pass.  grid (ceil(N / 256), heads, B), one token per lane: S again, ds = softmax backward of dS = (dY Vp) m2;
// g_qkvv slot 0 <- temperature2 ds Kp^T (dQh of the spatial branch); part[((b heads + h) ntile + tile)][2][D][P] = {sum_n (S m2)[n][p] dY[n][i],
// sum_n Qh[n][i] ds[n][p]} (Qh = Q / |q|, without temperature2), summed through an LDS stage of EPA_ST tokens per round.
template <int D, int P, bool MASK>
__global__ __launch_bounds__(EPA_NT) void cl_epa_bwd_tokens_kernel(const float *__restrict__ qkvv, const float *__restrict__ kp, const float *__restrict__ vp,
                                                                  const float *__restrict__ nrm, const float *__restrict__ temperature2,
                                                                  const unsigned char *__restrict__ m2, float m2_scale, const float *__restrict__ g_xsa,
                                                                  float *__restrict__ g_qkvv, float *__restrict__ part, int N, int C)
{
    constexpr int OUT = 2 * D * P / EPA_NT;   // outputs per lane of the partial tile
    static_assert(OUT * EPA_NT == 2 * D * P, "the partial tile divides over the workgroup");
    constexpr int PS = P + 1, DS = D + 1;     // row strides of the stage: the 16 lanes that fill it write one column each, an odd stride spreads them over the banks
    DLKA_DYN_SMEM(float, sm);   // sKp [D][P], sVp [D][P], stS [ST][PS], stDs [ST][PS], stQ [ST][DS], stDy [ST][DS], sRq [D]
    float *sKp = sm, *sVp = sm + D * P, *stS = sm + 2 * D * P, *stDs = stS + EPA_ST * PS, *stQ = stDs + EPA_ST * PS, *stDy = stQ + EPA_ST * DS, *sRq = stDy + EPA_ST * DS;
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z, heads = gridDim.y, ntile = gridDim.x;
    epa_load_head<D, P>(sKp, sVp, kp, vp, ((long)b * C + h * D) * P);
    if (tid < D) sRq[tid] = nrm[(long)b * 5 * C + h * D + tid];
    __syncthreads();
    const float t2 = temperature2[h];
    const int n = blockIdx.x * EPA_NT + tid;
    const bool live = n < N;
    float s[P], ds[P], qh[D], dy[D];
    if (live) {
        const float *row = qkvv + ((long)b * N + n) * 4 * C + h * D;
        {
            float qs[D];
#pragma unroll
            for (int i = 0; i < D; i += 4) {
                const f32x4 q = *reinterpret_cast<const f32x4 *>(row + i);
#pragma unroll
                for (int e = 0; e < 4; ++e) { qh[i + e] = q[e] * sRq[i + e]; qs[i + e] = qh[i + e] * t2; }
            }
            epa_token_softmax<D, P>(qs, sKp, s);
        }
        const float *gy = g_xsa + ((long)b * D * heads + h) * N + n;
#pragma unroll
        for (int i = 0; i < D; ++i) dy[i] = gy[(long)i * heads * N];
#pragma unroll
        for (int p = 0; p < P; ++p) ds[p] = 0.f;
#pragma unroll
        for (int i = 0; i < D; ++i) {
#pragma unroll
            for (int p = 0; p < P; p += 4) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(sVp + i * P + p);
                ds[p] = fmaf(dy[i], v[0], ds[p]); ds[p + 1] = fmaf(dy[i], v[1], ds[p + 1]); ds[p + 2] = fmaf(dy[i], v[2], ds[p + 2]); ds[p + 3] = fmaf(dy[i], v[3], ds[p + 3]);
            }
        }
        if (MASK) {
            float mult[P];
            epa_mask_row<P>(m2, (long)(b * heads + h) * N + n, m2_scale, mult);
            float dot = 0.f;
#pragma unroll
            for (int p = 0; p < P; ++p) { ds[p] *= mult[p]; dot = fmaf(s[p], ds[p], dot); }
#pragma unroll
            for (int p = 0; p < P; ++p) { ds[p] = s[p] * (ds[p] - dot); s[p] *= mult[p]; }
        } else {
            float dot = 0.f;
#pragma unroll
            for (int p = 0; p < P; ++p) dot = fmaf(s[p], ds[p], dot);
#pragma unroll
            for (int p = 0; p < P; ++p) ds[p] = s[p] * (ds[p] - dot);
        }
        float *gq = g_qkvv + ((long)b * N + n) * 4 * C + h * D;
#pragma unroll
        for (int i = 0; i < D; i += 4) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a = 0.f;
#pragma unroll
                for (int p = 0; p < P; p += 4) {
                    const f32x4 k = *reinterpret_cast<const f32x4 *>(sKp + (i + e) * P + p);
                    a = fmaf(ds[p], k[0], a); a = fmaf(ds[p + 1], k[1], a); a = fmaf(ds[p + 2], k[2], a); a = fmaf(ds[p + 3], k[3], a);
                }
                o[e] = a * t2;
            }
            *reinterpret_cast<f32x4 *>(gq + i) = o;
        }
    } else {
#pragma unroll
        for (int p = 0; p < P; ++p) s[p] = ds[p] = 0.f;
#pragma unroll
        for (int i = 0; i < D; ++i) qh[i] = dy[i] = 0.f;
    }
    float acc[OUT];
#pragma unroll
    for (int k = 0; k < OUT; ++k) acc[k] = 0.f;
    for (int r = 0; r < EPA_NT / EPA_ST; ++r) {
        __syncthreads();
        if (tid / EPA_ST == r) {
            const int t = tid % EPA_ST;
#pragma unroll
            for (int p = 0; p < P; ++p) { stS[t * PS + p] = s[p]; stDs[t * PS + p] = ds[p]; }
#pragma unroll
            for (int i = 0; i < D; ++i) { stQ[t * DS + i] = qh[i]; stDy[t * DS + i] = dy[i]; }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < OUT; ++k) {
            const int o = tid + k * EPA_NT;
            const bool second = o >= D * P;
            const int oo = second ? o - D * P : o, i = oo / P, p = oo % P;
            const float *u = second ? stQ : stDy, *v = second ? stDs : stS;
            float a = acc[k];
#pragma unroll
            for (int t = 0; t < EPA_ST; ++t) a = fmaf(u[t * DS + i], v[t * PS + p], a);
            acc[k] = a;
        }
    }
    float *out = part + ((long)(b * heads + h) * ntile + blockIdx.x) * 2 * D * P;
#pragma unroll
    for (int k = 0; k < OUT; ++k) out[tid + k * EPA_NT] = acc[k];
}

// One workgroup per (h, b).  Folds dA's partial Gram tiles (gpart, nchunk) and the token pass's tiles (tpart, ntile) in order.
//   g_vp <- sum_n (S m2) dY;  g_kp <- temperature2 sum_n Qh ds;  r_sa[i] = sum_p Kp[i][p] g_kp[i][p];  g_t2[b][h] = sum_i r_sa[i] / temperature2 (formed without the division)
//   dL = softmax backward of dA m1;  g_t[b][h] = sum dL ghat;  dgh = dL temperature[h]
//   proj[b][0][c] = (sum_j dgh[i][j] ghat[i][j] + r_sa[i]) * (|q_i| >= eps),  proj[b][1][c] = sum_i dgh[i][j] ghat[i][j] * (|k_j| >= eps)
template <int D, int P>
__global__ __launch_bounds__(EPA_NT) void cl_epa_bwd_finish_kernel(const float *__restrict__ gpart, int nchunk, const float *__restrict__ tpart, int ntile,
                                                                  const float *__restrict__ kp, const float *__restrict__ temperature,
                                                                  const float *__restrict__ temperature2, const float *__restrict__ m1,
                                                                  const float *__restrict__ a_soft, const float *__restrict__ ghat, const float *__restrict__ nrm,
                                                                  float *__restrict__ g_kp, float *__restrict__ g_vp, float *__restrict__ g_t, float *__restrict__ g_t2,
                                                                  float *__restrict__ dgh_out, float *__restrict__ proj, int C)
{
    constexpr int GF = epa_gram_floats(D);
    DLKA_DYN_SMEM(float, sm);   // dkp [D][P], w [D][D] (dgh ghat), rsa [D], raw [D], rowt [D]
    float *dkp = sm, *w = sm + D * P, *rsa = w + D * D, *raw = rsa + D, *rowt = raw + D;
    const int tid = threadIdx.x, h = blockIdx.x, b = blockIdx.y, heads = gridDim.x;
    const float t1 = temperature[h], t2 = temperature2[h];
    const long po = ((long)b * C + h * D) * P;
    const float *tp = tpart + (long)(b * heads + h) * ntile * 2 * D * P;
    for (int e = tid; e < 2 * D * P; e += EPA_NT) {
        float v = tp[e];
        for (int c = 1; c < ntile; ++c) v += tp[(long)c * 2 * D * P + e];
        if (e < D * P) g_vp[po + e] = v;
        else { dkp[e - D * P] = v; g_kp[po + e - D * P] = v * t2; }
    }
    __syncthreads();
    if (tid < D) {
        float r = 0.f;
        for (int p = 0; p < P; ++p) r = fmaf(kp[po + tid * P + p], dkp[tid * P + p], r);
        raw[tid] = r;
        rsa[tid] = r * t2;
    }
    const float *gp = gpart + (long)(b * heads + h) * nchunk * GF;
    const long ao = (long)(b * heads + h) * D * D;
    if (tid < D) {
        const int i = tid;
        float da[D], dot = 0.f;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            float v = gp[i * D + j];
            for (int c = 1; c < nchunk; ++c) v += gp[(long)c * GF + i * D + j];
            if (m1) v *= m1[ao + i * D + j];
            da[j] = v;
            dot = fmaf(a_soft[ao + i * D + j], v, dot);
        }
        float st = 0.f;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const float dl = a_soft[ao + i * D + j] * (da[j] - dot), gh = ghat[ao + i * D + j];
            st = fmaf(dl, gh, st);
            const float dg = dl * t1;
            dgh_out[ao + i * D + j] = dg;
            w[i * D + j] = dg * gh;
        }
        rowt[i] = st;
    }
    __syncthreads();
    const float *nb = nrm + (long)b * 5 * C;
    float *pb = proj + (long)b * 2 * C;
    if (tid < D) {
        float r = 0.f;
        for (int j = 0; j < D; ++j) r += w[tid * D + j];
        pb[h * D + tid] = (r + rsa[tid]) * nb[2 * C + h * D + tid];
    } else if (tid < 2 * D) {
        const int j = tid - D;
        float r = 0.f;
        for (int i = 0; i < D; ++i) r += w[i * D + j];
        pb[C + h * D + j] = r * nb[3 * C + h * D + j];
    } else if (tid == 2 * D) {
        float a = 0.f, c = 0.f;
        for (int i = 0; i < D; ++i) { a += rowt[i]; c += raw[i]; }
        g_t[b * heads + h] = a;
        g_t2[b * heads + h] = c;
    }
}

// Backward, second token pass.  grid (ceil(N / 256), heads, B), one token per lane: reads dQh of the spatial branch from slot 0 of g_qkvv and writes
// dQ (slot 0), dK (slot 1: the channel branch's part; Kp's comes through the projection), dVc (slot 2), zeros (slot 3).
template <int D>
__global__ __launch_bounds__(EPA_NT) void cl_epa_bwd_apply_kernel(const float *__restrict__ qkvv, const float *__restrict__ a_mask, const float *__restrict__ dgh,
                                                                 const float *__restrict__ nrm, const float *__restrict__ proj, const float *__restrict__ g_xca,
                                                                 float *__restrict__ g_qkvv, int N, int C)
{
    DLKA_DYN_SMEM(float, sm);   // sA [D][D], sG [D][D], sV [4][D] = {rq, rk, proj q, proj k}
    float *sA = sm, *sG = sm + D * D, *sV = sm + 2 * D * D;
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z, heads = gridDim.y;
    for (int e = tid; e < D * D; e += EPA_NT) { sA[e] = a_mask[(long)(b * heads + h) * D * D + e]; sG[e] = dgh[(long)(b * heads + h) * D * D + e]; }
    if (tid < D) {
        const float *nb = nrm + (long)b * 5 * C;
        sV[tid] = nb[h * D + tid];
        sV[D + tid] = nb[C + h * D + tid];
        sV[2 * D + tid] = proj[(long)b * 2 * C + h * D + tid];
        sV[3 * D + tid] = proj[(long)b * 2 * C + C + h * D + tid];
    }
    __syncthreads();
    const int n = blockIdx.x * EPA_NT + tid;
    if (n >= N) return;
    const float *row = qkvv + ((long)b * N + n) * 4 * C + h * D;
    float *grow = g_qkvv + ((long)b * N + n) * 4 * C + h * D;
    // one pass over the rows i of dgh and A (LDS rows are read once, as broadcasts); the sums over i stay in registers
    float kh[D], dk[D], dv[D];
#pragma unroll
    for (int j = 0; j < D; j += 4) {
        const f32x4 k = *reinterpret_cast<const f32x4 *>(row + C + j);
#pragma unroll
        for (int e = 0; e < 4; ++e) { kh[j + e] = k[e] * sV[D + j + e]; dk[j + e] = 0.f; dv[j + e] = 0.f; }
    }
    const float *gc = g_xca + ((long)b * N + n) * C + h * D;
#pragma unroll 2
    for (int i = 0; i < D; ++i) {
        const float qi = row[i] * sV[i], dxi = gc[i];
        float a = grow[i];
#pragma unroll
        for (int j = 0; j < D; j += 4) {
            const f32x4 g = *reinterpret_cast<const f32x4 *>(sG + i * D + j), w = *reinterpret_cast<const f32x4 *>(sA + i * D + j);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a = fmaf(g[e], kh[j + e], a);
                dk[j + e] = fmaf(g[e], qi, dk[j + e]);
                dv[j + e] = fmaf(w[e], dxi, dv[j + e]);
            }
        }
        grow[i] = sV[i] * (a - qi * sV[2 * D + i]);
    }
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < D; j += 4) {
        f32x4 o, v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = sV[D + j + e] * (dk[j + e] - kh[j + e] * sV[3 * D + j + e]);
            v[e] = dv[j + e];
        }
        *reinterpret_cast<f32x4 *>(grow + C + j) = o;
        *reinterpret_cast<f32x4 *>(grow + 2 * C + j) = v;
        *reinterpret_cast<f32x4 *>(grow + 3 * C + j) = zero;
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------------
int epa_gram_chunks(int N) { return cdiv(N, EPA_CHUNK); }
int epa_token_tiles(int N) { return cdiv(N, EPA_NT); }
size_t epa_gram_part_floats(int B, int N, int heads, int D) { return (size_t)B * heads * epa_gram_chunks(N) * epa_gram_floats(D); }
size_t epa_token_part_floats(int B, int N, int heads, int D, int P) { return (size_t)B * heads * epa_token_tiles(N) * 2 * D * P; }

template <class F> static bool epa_dispatch_d(int D, F &&f) { return dispatch_menu<8, 16, 32, 64>(D, f); }
template <class F> static bool epa_dispatch_p(int P, F &&f) { return dispatch_menu<32, 64>(P, f); }

int launch_cl_epa_gram(const float *X, long xb, int xs, int xo, const float *Y, long yb, int ys, int yo, float *part, int B, int N, int heads, int D, bool sumsq,
                       hipStream_t st)
{
    const int nchunk = epa_gram_chunks(N);
    const bool hit = epa_dispatch_d(D, [&](auto d) {
        constexpr int DD = DLKA_V(d);
        constexpr int T = epa_gram_tile(DD), S = EPA_NT / ((DD / T) * (DD / T));
        const size_t lds = (2 * EPA_GT * DD + S * epa_gram_floats(DD)) * sizeof(float);
        dispatch_bool(sumsq, [&](auto sq) {
            DLKA_LAUNCH((cl_epa_gram_kernel<DD, DLKA_V(sq)>), dim3(nchunk, heads, B), dim3(EPA_NT), lds, st, X, xb, xs, xo, Y, yb, ys, yo, part, N, nchunk);
        });
    });
    if (!hit) return DLKA_ERR_UNSUPPORTED;
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}

int launch_cl_epa_finish(const float *part, const float *temperature, const float *temperature2, const float *m1, float *nrm, float *ghat, float *a_soft,
                         float *a_mask, int B, int N, int C, int heads, hipStream_t st)
{
    const bool hit = epa_dispatch_d(C / heads, [&](auto d) {
        DLKA_LAUNCH((cl_epa_finish_kernel<DLKA_V(d)>), dim3(heads, B), dim3(EPA_NT), 0, st, part, epa_gram_chunks(N), temperature, temperature2, m1, nrm, ghat,
                    a_soft, a_mask, C);
    });
    if (!hit) return DLKA_ERR_UNSUPPORTED;
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}

int launch_cl_epa_apply(const float *qkvv, const float *kp, const float *vp, const float *a_mask, const float *nrm, const unsigned char *m2, float m2_scale,
                        float *x_sa, float *x_ca, int B, int N, int C, int heads, int P, hipStream_t st)
{
    bool hit = false;
    epa_dispatch_d(C / heads, [&](auto d) {
        hit = epa_dispatch_p(P, [&](auto p) {
            constexpr int DD = DLKA_V(d), PP = DLKA_V(p);
            const size_t lds = (2 * DD * PP + DD * DD + DD) * sizeof(float);
            dispatch_bool(m2 != nullptr, [&](auto mk) {
                DLKA_LAUNCH((cl_epa_apply_kernel<DD, PP, DLKA_V(mk)>), dim3(epa_token_tiles(N), heads, B), dim3(EPA_NT), lds, st, qkvv, kp, vp, a_mask, nrm, m2,
                            m2_scale, x_sa, x_ca, N, C);
            });
        });
    });
    if (!hit) return DLKA_ERR_UNSUPPORTED;
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}

int launch_cl_epa_bwd_tokens(const float *qkvv, const float *kp, const float *vp, const float *nrm, const float *temperature2, const unsigned char *m2,
                             float m2_scale, const float *g_xsa, float *g_qkvv, float *part, int B, int N, int C, int heads, int P, hipStream_t st)
{
    bool hit = false;
    epa_dispatch_d(C / heads, [&](auto d) {
        hit = epa_dispatch_p(P, [&](auto p) {
            constexpr int DD = DLKA_V(d), PP = DLKA_V(p);
            const size_t lds = (2 * DD * PP + 2 * EPA_ST * (PP + 1) + 2 * EPA_ST * (DD + 1) + DD) * sizeof(float);
            dispatch_bool(m2 != nullptr, [&](auto mk) {
                DLKA_LAUNCH((cl_epa_bwd_tokens_kernel<DD, PP, DLKA_V(mk)>), dim3(epa_token_tiles(N), heads, B), dim3(EPA_NT), lds, st, qkvv, kp, vp, nrm,
                            temperature2, m2, m2_scale, g_xsa, g_qkvv, part, N, C);
            });
        });
    });
    if (!hit) return DLKA_ERR_UNSUPPORTED;
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}

int launch_cl_epa_bwd_finish(const float *gpart, const float *tpart, const float *kp, const float *temperature, const float *temperature2, const float *m1,
                             const float *a_soft, const float *ghat, const float *nrm, float *g_kp, float *g_vp, float *g_t, float *g_t2, float *dgh, float *proj,
                             int B, int N, int C, int heads, int P, hipStream_t st)
{
    bool hit = false;
    epa_dispatch_d(C / heads, [&](auto d) {
        hit = epa_dispatch_p(P, [&](auto p) {
            constexpr int DD = DLKA_V(d), PP = DLKA_V(p);
            const size_t lds = (DD * PP + DD * DD + 3 * DD) * sizeof(float);
            DLKA_LAUNCH((cl_epa_bwd_finish_kernel<DD, PP>), dim3(heads, B), dim3(EPA_NT), lds, st, gpart, epa_gram_chunks(N), tpart, epa_token_tiles(N), kp,
                        temperature, temperature2, m1, a_soft, ghat, nrm, g_kp, g_vp, g_t, g_t2, dgh, proj, C);
        });
    });
    if (!hit) return DLKA_ERR_UNSUPPORTED;
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}

int launch_cl_epa_bwd_apply(const float *qkvv, const float *a_mask, const float *dgh, const float *nrm, const float *proj, const float *g_xca, float *g_qkvv, int B,
                            int N, int C, int heads, hipStream_t st)
{
    const bool hit = epa_dispatch_d(C / heads, [&](auto d) {
        constexpr int DD = DLKA_V(d);
        const size_t lds = (2 * DD * DD + 4 * DD) * sizeof(float);
        DLKA_LAUNCH((cl_epa_bwd_apply_kernel<DD>), dim3(epa_token_tiles(N), heads, B), dim3(EPA_NT), lds, st, qkvv, a_mask, dgh, nrm, proj, g_xca, g_qkvv, N, C);
    });
    if (!hit) return DLKA_ERR_UNSUPPORTED;
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}

}  // namespace dlka
