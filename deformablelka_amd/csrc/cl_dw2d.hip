// Channels-last depthwise 2-D convolution with bias: the two large-kernel convs of the plain (non-deformable) 2-D LKA block, 5x5 pad 2 and 7x7 dilation 3
// pad 9 (2D/deformable_LKA/LKA.py:7-8; cuDNN in the reference).  [B][H][W][C], C a multiple of 32, activations float or bf16 storage with fp32 arithmetic.
//
// No contraction over channels, so — as in cl_dwconv.hip — a register-tiled vector kernel: 32 lanes run over 32 consecutive channels (one 128-byte piece of a
// pixel's channel row per load), a work-item owns TW consecutive outputs along W of one row and slides the K taps of each tap row over one input row segment
// held in registers (TW + (K - 1) * DIL loads feed TW * K FMAs).  A workgroup is eight such 32-lane units; consecutive units are the channel groups of one
// pixel run, so the loads of a wave stay contiguous for C >= 64.
//
// Bounds.  Every activation load goes through ONE buffer descriptor over the whole tensor; an element outside its image — a tap row above or below it (skipped
// as a whole), a tap column left or right of the row — gets the byte offset 0xffffffff, which the hardware range check answers with 0.  The row test is against
// the image's own H, the column test against W, so no read crosses from one image of the batch into the next or from one row into its neighbour.
//
// The data gradient of a stride-1 "same" conv is the same conv with flipped taps and no bias: the same kernel on the flipped prepared weights.
//
// Weight and bias gradient: per-workgroup partial tiles part[chunk][tap][c] and bpart[chunk][c], summed in a fixed order inside the workgroup (LDS, slot 0 .. 7)
// and folded over the chunks by cl_wgrad.hip's finalisation (a FinalizeJob of kind 0 with Cin = 1) — no float atomics, bitwise reproducible.
#include "cl_args.h"
#include "dlka_kernels.h"

namespace dlka {

constexpr int DW2D_TW = 8;            // outputs along W per work-item
constexpr unsigned DW2D_OOB = 0xffffffffu;

template <typename T, int K, int DIL, int TW>
__global__ __launch_bounds__(256) void cl_dw2d_kernel(Dw2dArgs p)
{
    constexpr int P = DIL * (K - 1) / 2, SEG = TW + (K - 1) * DIL, SB = sizeof(T);
    const int CG = p.C >> 5, lane = threadIdx.x & 31;
    const int runs_per_row = cdiv(p.W, TW);
    const long unit = (long)blockIdx.x * 8 + (threadIdx.x >> 5);
    if (unit >= (long)p.B * p.H * runs_per_row * CG) return;
    const int c = (int)(unit % CG) * 32 + lane;
    const long run = unit / CG;
    const int w0 = (int)(run % runs_per_row) * TW;
    const int row = (int)(run / runs_per_row);       // b * H + h0
    const int h0 = row % p.H, b = row / p.H;
    T *outp = reinterpret_cast<T *>(p.out);
    const BufRsrc rin = make_rsrc(p.in, (size_t)p.B * p.H * p.W * p.C * SB);   // (< 2^31 bytes: the launcher checks)

    float acc[TW];
    const float bv = p.bias ? p.bias[c] : 0.f;
#pragma unroll
    for (int t = 0; t < TW; ++t) acc[t] = bv;

#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int zh = h0 + j * DIL - P;
        if ((unsigned)zh >= (unsigned)p.H) continue;                      // a tap row outside THIS image
        const unsigned rowoff = (unsigned)(((b * p.H + zh) * p.W) * p.C + c) * SB;
        float seg[SEG];
#pragma unroll
        for (int e = 0; e < SEG; ++e) {
            const int zw = w0 - P + e;
            seg[e] = act_buf_load1<T>(rin, (unsigned)zw < (unsigned)p.W ? rowoff + (unsigned)(zw * p.C) * SB : DW2D_OOB);
        }
        const float *wrow = p.wp + (long)(j * K) * p.C + c;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float wv = wrow[(long)k * p.C];
#pragma unroll
            for (int t = 0; t < TW; ++t) acc[t] = fmaf(wv, seg[t + k * DIL], acc[t]);
        }
    }
    const long obase = ((long)row * p.W + w0) * p.C + c;
#pragma unroll
    for (int t = 0; t < TW; ++t)
        if (w0 + t < p.W) act_store1(outp, obase + (long)t * p.C, acc[t]);
}

// gW[c][j][k] = sum_{b,h,w} G[b,h,w][c] * in[b, h + j*DIL - P, w + k*DIL - P][c];  gb[c] = sum G[b,h,w][c].
// grid = (chunks, C / 32).  A workgroup owns the pixel runs [chunk * runs_per_chunk, +runs_per_chunk) of one 32-channel group; its eight 32-lane slots stride
// over them with K*K accumulators each, and the slots' sums meet in LDS in slot order.  Every workgroup writes its whole tile (zeros where it had no run).
template <typename T, int K, int DIL, int TW>
__global__ __launch_bounds__(256) void cl_dw2d_wgrad_kernel(Dw2dWgradArgs p)
{
    constexpr int P = DIL * (K - 1) / 2, SEG = TW + (K - 1) * DIL, SB = sizeof(T);
    __shared__ float red[8][8][32];   // [k | bias][slot][lane]
    const int lane = threadIdx.x & 31, slot = threadIdx.x >> 5;
    const int c = blockIdx.y * 32 + lane;
    const int runs_per_row = cdiv(p.W, TW);
    const long runs = (long)p.B * p.H * runs_per_row;
    const long run_lo = (long)blockIdx.x * p.runs_per_chunk;
    const long run_hi = run_lo + p.runs_per_chunk < runs ? run_lo + p.runs_per_chunk : runs;
    const size_t bytes = (size_t)p.B * p.H * p.W * p.C * SB;
    const BufRsrc rin = make_rsrc(p.in, bytes), rg = make_rsrc(p.g, bytes);

    float acc[K][K];
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
        for (int k = 0; k < K; ++k) acc[j][k] = 0.f;
    float bsum = 0.f;
    for (long run = run_lo + slot; run < run_hi; run += 8) {
        const int w0 = (int)(run % runs_per_row) * TW;
        const int row = (int)(run / runs_per_row);
        const int h0 = row % p.H, b = row / p.H;
        const unsigned goff = (unsigned)((row * p.W + w0) * p.C + c) * SB;
        float gv[TW];
#pragma unroll
        for (int t = 0; t < TW; ++t) gv[t] = act_buf_load1<T>(rg, w0 + t < p.W ? goff + (unsigned)(t * p.C) * SB : DW2D_OOB);
#pragma unroll
        for (int t = 0; t < TW; ++t) bsum += gv[t];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int zh = h0 + j * DIL - P;
            if ((unsigned)zh >= (unsigned)p.H) continue;
            const unsigned rowoff = (unsigned)(((b * p.H + zh) * p.W) * p.C + c) * SB;
            float seg[SEG];
#pragma unroll
            for (int e = 0; e < SEG; ++e) {
                const int zw = w0 - P + e;
                seg[e] = act_buf_load1<T>(rin, (unsigned)zw < (unsigned)p.W ? rowoff + (unsigned)(zw * p.C) * SB : DW2D_OOB);
            }
#pragma unroll
            for (int k = 0; k < K; ++k)
#pragma unroll
                for (int t = 0; t < TW; ++t) acc[j][k] = fmaf(gv[t], seg[t + k * DIL], acc[j][k]);
        }
    }
    float *tile = p.part + (size_t)blockIdx.x * K * K * p.C;
#pragma unroll
    for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[k][slot][lane] = acc[j][k];
        if (j == 0) red[7][slot][lane] = bsum;      // (K <= 7: row 7 is free)
        __syncthreads();
        if (slot < K) {                             // slot s folds tap (j, s) over the eight slots, in slot order
            float a = 0.f;
#pragma unroll
            for (int s = 0; s < 8; ++s) a += red[slot][s][lane];
            tile[(size_t)(j * K + slot) * p.C + c] = a;
        } else if (j == 0 && slot == 7 && p.bpart) {
            float a = 0.f;
#pragma unroll
            for (int s = 0; s < 8; ++s) a += red[7][s][lane];
            p.bpart[(size_t)blockIdx.x * p.C + c] = a;
        }
        __syncthreads();
    }
}

static bool dw2d_shape(int k, int dil) { return (k == 5 && dil == 1) || (k == 7 && dil == 3); }

bool cl_dw2d_supported(int B, int H, int W, int C, int k, int dil)
{
    return B > 0 && H > 0 && W > 0 && C > 0 && C % 32 == 0 && dw2d_shape(k, dil) && (long)B * H * W * C < (1l << 29);   // byte offsets of fp32 elements stay below 2^31
}

int launch_cl_dw2d(const Dw2dArgs &a, int k, int dil, hipStream_t st)
{
    if (!cl_dw2d_supported(a.B, a.H, a.W, a.C, k, dil)) return DLKA_ERR_UNSUPPORTED;
    const long units = (long)a.B * a.H * cdiv(a.W, DW2D_TW) * (a.C / 32);
    const dim3 grid((unsigned)cdivl(units, 8)), block(256);
    dispatch_act(a.act_bf16 != 0, [&](auto t) { dispatch_bool(k == 7, [&](auto k7) {
        auto kern = cl_dw2d_kernel<DLKA_T(t), DLKA_V(k7) ? 7 : 5, DLKA_V(k7) ? 3 : 1, DW2D_TW>;
        DLKA_LAUNCH(kern, grid, block, 0, st, a);
    }); });
    DLKA_CHECK_LAUNCH();
    return DLKA_OK;
}

// pixel runs per workgroup: at least 16 (two per slot), and no more than 256 partial tiles
static int dw2d_runs_per_chunk(int B, int H, int W)
{
    const long runs = (long)B * H * cdiv(W, DW2D_TW);
    const long rpc = cdivl(runs, 256) > 16 ? cdivl(runs, 256) : 16;
    return (int)(cdivl(rpc, 8) * 8);
}
int cl_dw2d_wgrad_chunks(int B, int H, int W) { return (int)cdivl((long)B * H * cdiv(W, DW2D_TW), dw2d_runs_per_chunk(B, H, W)); }
size_t cl_dw2d_part_floats(int B, int H, int W, int C, int k) { return (size_t)cl_dw2d_wgrad_chunks(B, H, W) * (k * k + 1) * C; }

// a.part: cl_dw2d_part_floats() floats.  The partial tiles are written here; `fold` is filled in for launch_cl_wgrad_finalize, which writes gw [C][1][k][k] and gb [C] (or null).
int launch_cl_dw2d_wgrad(Dw2dWgradArgs a, int k, int dil, float *gw, float *gb, hipStream_t st, FinalizeJob *fold)
{
    if (!cl_dw2d_supported(a.B, a.H, a.W, a.C, k, dil) || !fold || !gw) return DLKA_ERR_UNSUPPORTED;
    a.runs_per_chunk = dw2d_runs_per_chunk(a.B, a.H, a.W);
    a.chunks = cl_dw2d_wgrad_chunks(a.B, a.H, a.W);
    a.bpart = gb ? a.part + (size_t)a.chunks * k * k * a.C : nullptr;
    const dim3 grid(a.chunks, a.C / 32), block(256);
    dispatch_act(a.act_bf16 != 0, [&](auto t) { dispatch_bool(k == 7, [&](auto k7) {
        auto kern = cl_dw2d_wgrad_kernel<DLKA_T(t), DLKA_V(k7) ? 7 : 5, DLKA_V(k7) ? 3 : 1, DW2D_TW>;
        DLKA_LAUNCH(kern, grid, block, 0, st, a);
    }); });
    DLKA_CHECK_LAUNCH();
    memset(fold, 0, sizeof(*fold));
    fold->part = a.part; fold->bpart = a.bpart; fold->gw = gw; fold->gb = gb;
    fold->chunks = a.chunks; fold->K = k * k; fold->CoutP = a.C; fold->Cout = a.C; fold->Cin = 1; fold->kind = 0;
    fold->n = (long)k * k * a.C + (gb ? a.C : 0);
    return DLKA_OK;
}

}  // namespace dlka
