// The frame the channels-last 2-D attention blocks share.  Both compute   y = proj_2( a * conv1( S(a) ) ) + x,   a = GELU(proj_1 x),   on [B][H][W][C] tensors
// between one transpose in and one transpose out; only the spatial stage S differs (capi_lka2d_cl.hip: offset nets + deformable depthwise convs;
// capi_lka2d_plain_cl.hip: depthwise 5x5, then 7x7 dilation 3).  Written ONCE here: the pointwise geometry, the saved activations, the six prepared pointwise
// weights, the width menu, the launches in front of and behind S in both directions.
// RULE: a change to the pointwise frame is made in this header; a block file holds only its spatial stage and its buffers.
#pragma once
#include "cl_host.h"

namespace dlka {

inline SameConv block_conv2d(int B, int C, int Cout, int H, int W, int k, int pad, int dil, int act_bf16 = 0)
{
    SameConv s;
    s.act_bf16 = act_bf16;
    s.B = B; s.D = 1; s.H = H; s.W = W; s.N = H * W; s.M = B * s.N; s.Cin = C; s.Cout = Cout; s.group = 1;
    s.kd = 1; s.kh = s.kw = k; s.pd = 0; s.ph = s.pw = pad; s.dd = 1; s.dh = s.dw = dil; s.K = k * k;
    return s;
}

// The width menu, C / 32 in {1, 2, 3, 4, 6, 8, 12}: the column tiles the pointwise kernel has.  (The deformable block also keeps its own conditions:
// cl_ddw2d_supported, the same seven widths, and nt_ok(C) || C == 192 || C == 384, which holds for all seven — neither accepts a width the menu refuses.)
inline bool frame_width_ok(int C) { const int ct = C / 32; return C > 0 && C % 32 == 0 && (ct <= 4 || ct == 6 || ct == 8 || ct == 12); }

struct Lka2dFrame {
    int B, C, H, W, bf;
    size_t E, SB;         // elements of one activation tensor, bytes of one stored element
    SameConv pw;          // the three pointwise convs; activation-typed (bf16 storage on DLKA_BF16)
    Lka2dFrame(int B_, int C_, int H_, int W_, int dtype)
        : B(B_), C(C_), H(H_), W(W_), bf(dtype == DLKA_BF16), E((size_t)B * C * H * W), SB(bf ? 2 : 4), pw(block_conv2d(B, C, C, H, W, 1, 0, 1, bf)) {}
    size_t pw_floats() const { return (size_t)C * C; }
    size_t part_pw() const { return (cl_wgrad_part_floats_mode(pw.M, 1, C, C, 0) + 63) & ~(size_t)63; }
};

// the activation-typed tensors at the head of both blocks' `saved`: t1 = the first spatial conv's output, t2 = S(a), g1 = conv1(t2), m = a * g1
struct FrameSaved {
    float *xt, *h, *a, *t1, *t2, *g1, *m;
    void carve(Carver &sv, const Lka2dFrame &G) { for (float **t : {&xt, &h, &a, &t1, &t2, &g1, &m}) *t = (float *)sv.take(G.E * G.SB); }
};

// the prepared weights inside `saved`, handed out by a bump pointer in 64-float steps: the three pointwise convs (forward / data-gradient form) come first,
// in the order proj_1, conv1, proj_2, with their jobs; each block carves its own weights behind them
struct PrepTake { float *q; float *operator()(size_t n) { float *r = q; q += (n + 63) & ~(size_t)63; return r; } };
struct FramePrep { float *pw_f[3], *pw_b[3]; };
template <class P>
void carve_frame_prep(const Lka2dFrame &G, PrepTake &take, FramePrep &t, const P *p, PrepBatch &pb)
{
    const void *pw_w[3] = {p->proj_1_w, p->conv1_w, p->proj_2_w};
    for (int k = 0; k < 3; ++k) {
        t.pw_f[k] = take(G.pw_floats()); t.pw_b[k] = take(G.pw_floats());
        add_job(pb, pw_w[k], t.pw_f[k], G.C, G.C, 1, G.C, G.C, 0);
        add_job(pb, pw_w[k], t.pw_b[k], G.C, G.C, 1, G.C, G.C, 1);
    }
}

// NCHW -> NHWC, then proj_1 + GELU: h, a (a32: + an fp32 copy of a, the deformable block's bf16 path)
inline int frame_forward_head(const Lka2dFrame &G, const FramePrep &PW, const void *x, const void *proj_1_b, const FrameSaved &S, float *a32, hipStream_t st)
{
    DLKA_TRY(launch_cl_transpose((const float *)x, S.xt, G.B, G.C, G.pw.N, 1, st, G.bf));
    return dense_forward(G.pw, S.xt, nullptr, (const float *)proj_1_b, S.h, 0, PW.pw_f[0], 1, nullptr, S.a, st, false, nullptr, a32);
}
// conv1 + gate (m = a * g1), proj_2 + shortcut, NHWC -> NCHW
inline int frame_forward_tail(const Lka2dFrame &G, const FramePrep &PW, const void *conv1_b, const void *proj_2_b, const FrameSaved &S, float *yt, void *y, hipStream_t st)
{
    DLKA_TRY(dense_forward(G.pw, S.t2, nullptr, (const float *)conv1_b, S.g1, 0, PW.pw_f[1], 2, S.a, S.m, st));
    DLKA_TRY(dense_forward(G.pw, S.m, nullptr, (const float *)proj_2_b, yt, 0, PW.pw_f[2], 3, S.xt, nullptr, st));
    return launch_cl_transpose(yt, (float *)y, G.B, G.C, G.pw.N, 0, st, G.bf);
}

// transpose grad_y; proj_2 data gradient with the gate's backward in the epilogue: gg1 = gm * a, ga1 = gm * g1; conv1 data gradient: gt2
inline int frame_backward_head(const Lka2dFrame &G, const FramePrep &PW, const FrameSaved &S, const void *grad_y, float *gyt, float *gg1, float *ga1, float *gt2, hipStream_t st)
{
    DLKA_TRY(launch_cl_transpose((const float *)grad_y, gyt, G.B, G.C, G.pw.N, 1, st, G.bf));
    DLKA_TRY(dense_backward_data(G.pw, gyt, 0, nullptr, gg1, PW.pw_b[2], 4, S.a, st, S.g1, ga1));
    return dense_backward_data(G.pw, gg1, 0, nullptr, gt2, PW.pw_b[1], 0, nullptr, st);
}
// behind S, which left gas = dL/da through S: gh = (ga1 + gas) * gelu'(h), then the three pointwise weight gradients (part[] = proj_2, conv1, proj_1), folds appended to `fb`
template <class Gr>
int frame_backward_wgrads(const Lka2dFrame &G, const FrameSaved &S, const Gr *gr, const float *gyt, const float *gg1, const float *ga1, const float *gas, float *gh,
                          float *const part[3], FinalizeBatch &fb, hipStream_t st)
{
    if (G.bf) DLKA_TRY(launch_gelu_bwd_sum<bf16_t>((const bf16_t *)S.h, (const bf16_t *)ga1, (const bf16_t *)gas, (bf16_t *)gh, (long)G.E, st));
    else DLKA_TRY(launch_gelu_bwd_sum<float>(S.h, ga1, gas, gh, (long)G.E, st));
    WgradArgs jobs[3];
    fill_pw_wgrad(jobs[0], G.pw, S.m, gyt, part[0]);
    fill_pw_wgrad(jobs[1], G.pw, S.t2, gg1, part[1]);
    fill_pw_wgrad(jobs[2], G.pw, S.xt, gh, part[2]);
    float *const gws[3] = {(float *)gr->proj_2_w, (float *)gr->conv1_w, (float *)gr->proj_1_w};
    float *const gbs[3] = {(float *)gr->proj_2_b, (float *)gr->conv1_b, (float *)gr->proj_1_b};
    fb.njobs += 3;
    return launch_cl_wgrad_pw3(jobs, gws, gbs, st, &fb.j[fb.njobs - 3]);
}
// ... and, once every partial sum `fb` folds is complete on `st` (the deformable block joins its internal stream in between): the folds, gx = P1^T gh + gy, NHWC -> NCHW
inline int frame_backward_finish(const Lka2dFrame &G, const FramePrep &PW, FinalizeBatch &fb, const float *gyt, const float *gh, float *gxt, void *grad_x, hipStream_t st)
{
    DLKA_TRY(launch_cl_wgrad_finalize(fb, st));
    DLKA_TRY(dense_backward_data(G.pw, gh, 0, nullptr, gxt, PW.pw_b[0], 3, gyt, st));
    return launch_cl_transpose(gxt, (float *)grad_x, G.B, G.C, G.pw.N, 0, st, G.bf);
}

}  // namespace dlka
