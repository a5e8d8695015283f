// =========================================================================================================================
// The plain (non-deformable) 2-D LKA block (LKA_Attention, 2D/deformable_LKA/LKA.py:21-37; SpatialAttention of 2D/networks/MaxViT_LKA_Decoder.py:69-85)
// on the channels-last kernels:   y = proj_2( u * conv1( conv_spatial( conv0(u) ) ) ) + x,   u = GELU(proj_1 x).
// x / y arrive in the reference's NCHW layout; the block transposes once on the way in and once on the way out and runs entirely in [B][H][W][C]:
//   1x1 projections (+GELU / gate / residual epilogues)      cl_pointwise_kernel, as in capi_lka2d_cl.hip
//   depthwise 5x5 and 7x7 dilation 3, both with bias         cl_dw2d.hip (forward, data gradient on flipped taps, weight + bias gradient in partial tiles)
// Supported: fp32 and DLKA_BF16 (bf16 activations, fp32 parameters and accumulation), C / 32 in {1, 2, 3, 4, 6, 8, 12}; anything else DLKA_ERR_UNSUPPORTED.
// No float atomics anywhere in the block: two identical calls give the same bits.
// Also here: the two depthwise convs as single operators (dlka_dwconv2d_*_cl), for the tests that hold cl_dw2d.hip against a reference on its own.
// =========================================================================================================================
#include "cl_host.h"

using namespace dlka;

namespace dlka {

namespace {

struct LkaPlainCl {
    SameConv pw;
    size_t E, SB;
    int B, C, H, W, bf;
    LkaPlainCl(int B_, int C_, int H_, int W_, int dtype) : B(B_), C(C_), H(H_), W(W_)
    {
        bf = dtype == DLKA_BF16 ? 1 : 0;
        SB = bf ? 2 : 4;
        SameConv &s = pw;
        s.act_bf16 = bf;
        s.B = B; s.D = 1; s.H = H; s.W = W; s.N = H * W; s.M = B * s.N; s.Cin = C; s.Cout = C; s.group = 1;
        s.kd = s.kh = s.kw = 1; s.pd = s.ph = s.pw = 0; s.dd = s.dh = s.dw = 1; s.K = 1;
        E = (size_t)B * C * H * W;
    }
    size_t pw_floats() const { return (size_t)C * C; }
    size_t prep_floats() const { return 6 * (pw_floats() + 64) + 2 * ((size_t)25 * C + 64) + 2 * ((size_t)49 * C + 64); }
    size_t part_pw() const { return (cl_wgrad_part_floats_mode(pw.M, 1, C, C, 0) + 63) & ~(size_t)63; }
    size_t part_dw(int k) const { return (cl_dw2d_part_floats(B, H, W, C, k) + 63) & ~(size_t)63; }
};

// prepared weights: the three pointwise convs (forward / data-gradient form), the two depthwise convs (forward / flipped taps)
struct PrepPlain { float *pw_f[3], *pw_b[3], *dw5, *dw5_b, *dw7, *dw7_b; };

int carve_prep_plain(const LkaPlainCl &G, float *base, PrepPlain &t, const dlka_lka2d_plain_params *p, hipStream_t st, bool fill)
{
    float *q = base;
    auto take = [&](size_t n) { float *r = q; q += (n + 63) & ~(size_t)63; return r; };
    for (int k = 0; k < 3; ++k) { t.pw_f[k] = take(G.pw_floats()); t.pw_b[k] = take(G.pw_floats()); }
    t.dw5 = take((size_t)25 * G.C); t.dw5_b = take((size_t)25 * G.C);
    t.dw7 = take((size_t)49 * G.C); t.dw7_b = take((size_t)49 * G.C);
    if (!fill) return DLKA_OK;
    PrepBatch pb;
    memset(&pb, 0, sizeof(pb));
    const int C = G.C;
    const void *pw_w[3] = {p->proj_1_w, p->conv1_w, p->proj_2_w};
    for (int k = 0; k < 3; ++k) {
        add_job(pb, pw_w[k], t.pw_f[k], C, C, 1, C, C, 0);
        add_job(pb, pw_w[k], t.pw_b[k], C, C, 1, C, C, 1);
    }
    add_job(pb, p->conv0_w, t.dw5, C, C, 25, 0, 0, 3);
    add_job(pb, p->conv0_w, t.dw5_b, C, C, 25, 0, 0, 4);
    add_job(pb, p->conv_spatial_w, t.dw7, C, C, 49, 0, 0, 3);
    add_job(pb, p->conv_spatial_w, t.dw7_b, C, C, 49, 0, 0, 4);
    return launch_cl_prep_batch(pb, st);
}

// ---- the block's buffer layouts: one record and one carve function per buffer and direction (Carver, cl_host.h) ----------------------------------
struct LkaPlainSaved { float *xt, *h, *a, *t1, *t2, *g1, *m, *prep; };   // activation-typed tensors, then the prepared weights
LkaPlainSaved carve_plain_saved(Carver &sv, const LkaPlainCl &G)
{
    LkaPlainSaved S;
    float **act[7] = {&S.xt, &S.h, &S.a, &S.t1, &S.t2, &S.g1, &S.m};
    for (float **t : act) *t = (float *)sv.take(G.E * G.SB);
    S.prep = (float *)sv.take(G.prep_floats() * 4);
    return S;
}
struct LkaPlainFwdWs { float *yt; };
LkaPlainFwdWs carve_plain_fwd_ws(Carver &cv, const LkaPlainCl &G)
{
    LkaPlainFwdWs W;
    W.yt = (float *)cv.take(G.E * G.SB);
    return W;
}
struct LkaPlainBwdWs {
    float *gyt, *gg1, *ga1, *gt2, *gt1, *gaa, *gh, *gxt;
    float *part_p2, *part_c1, *part_p1, *part_d7, *part_d5;
};
LkaPlainBwdWs carve_plain_bwd_ws(Carver &cv, const LkaPlainCl &G)
{
    LkaPlainBwdWs W;
    float **grad[8] = {&W.gyt, &W.gg1, &W.ga1, &W.gt2, &W.gt1, &W.gaa, &W.gh, &W.gxt};
    for (float **g : grad) *g = (float *)cv.take(G.E * G.SB);
    W.part_p2 = (float *)cv.take(G.part_pw() * 4); W.part_c1 = (float *)cv.take(G.part_pw() * 4); W.part_p1 = (float *)cv.take(G.part_pw() * 4);
    W.part_d7 = (float *)cv.take(G.part_dw(7) * 4); W.part_d5 = (float *)cv.take(G.part_dw(5) * 4);
    return W;
}

int plain_supported(int B, int C, int H, int W, int dtype)
{
    if ((dtype != DLKA_F32 && dtype != DLKA_BF16) || B <= 0 || C <= 0 || H <= 0 || W <= 0 || C % 32 != 0) return 0;
    const int ct = C / 32;
    if (!(ct == 1 || ct == 2 || ct == 3 || ct == 4 || ct == 6 || ct == 8 || ct == 12)) return 0;
    return cl_dw2d_supported(B, H, W, C, 5, 1) ? 1 : 0;   // (these widths are the pointwise kernel's menu, as in capi_lka2d_cl.hip)
}

int dw2d(const LkaPlainCl &G, const float *in, const float *wp, const void *bias, float *out, int k, int dil, hipStream_t st)
{
    Dw2dArgs d;
    memset(&d, 0, sizeof(d));
    d.in = in; d.wp = wp; d.bias = (const float *)bias; d.out = out; d.B = G.B; d.H = G.H; d.W = G.W; d.C = G.C; d.act_bf16 = G.bf;
    return launch_cl_dw2d(d, k, dil, st);
}

int dw2d_wgrad(const LkaPlainCl &G, const float *in, const float *g, float *part, void *gw, void *gb, int k, int dil, hipStream_t st, FinalizeJob *fold)
{
    Dw2dWgradArgs d;
    memset(&d, 0, sizeof(d));
    d.in = in; d.g = g; d.part = part; d.B = G.B; d.H = G.H; d.W = G.W; d.C = G.C; d.act_bf16 = G.bf;
    return launch_cl_dw2d_wgrad(d, k, dil, (float *)gw, (float *)gb, st, fold);
}

// ---- the single operators ---------------------------------------------------------------------------------------------------------------------
struct Dw2dOp { int B, H, W, C, k, dil; };
int make_dw2d_op(const dlka_conv_geom *c, int dtype, Dw2dOp &o)
{
    if (!c) return DLKA_ERR_NULL;
    if (dtype != DLKA_F32 && dtype != DLKA_BF16) return DLKA_ERR_UNSUPPORTED;
    if (c->B <= 0 || c->C <= 0 || c->H <= 0 || c->W <= 0 || c->kh <= 0 || c->kw <= 0 || c->dh <= 0 || c->dw <= 0) return DLKA_ERR_SHAPE;
    if (c->D != 1 || c->kd != 1 || c->sd != 1 || c->dd != 1 || c->pd != 0) return DLKA_ERR_SHAPE;
    if (c->group != c->C || c->Cout != c->C || c->sh != 1 || c->sw != 1 || c->kh != c->kw || c->dh != c->dw || c->ph != c->pw) return DLKA_ERR_UNSUPPORTED;
    if (c->ph != c->dh * (c->kh - 1) / 2 || !cl_dw2d_supported(c->B, c->H, c->W, c->C, c->kh, c->dh)) return DLKA_ERR_UNSUPPORTED;
    o.B = c->B; o.H = c->H; o.W = c->W; o.C = c->C; o.k = c->kh; o.dil = c->dh;
    return DLKA_OK;
}

}  // namespace
}  // namespace dlka

extern "C" {

size_t dlka_lka2d_plain_saved_bytes(int B, int C, int H, int W, int dtype)
{
    if (!plain_supported(B, C, H, W, dtype)) return 0;
    const LkaPlainCl G(B, C, H, W, dtype);
    return carved_bytes([&](Carver &m) { carve_plain_saved(m, G); });
}

size_t dlka_lka2d_plain_workspace_bytes(int B, int C, int H, int W, int dtype)
{
    if (!plain_supported(B, C, H, W, dtype)) return 0;
    const LkaPlainCl G(B, C, H, W, dtype);
    const size_t f = carved_bytes([&](Carver &m) { carve_plain_fwd_ws(m, G); }), b = carved_bytes([&](Carver &m) { carve_plain_bwd_ws(m, G); });
    return f > b ? f : b;
}

int dlka_lka2d_plain_attention_forward(const void *x, const dlka_lka2d_plain_params *p, void *y, void *saved, size_t saved_bytes, void *workspace,
                                       size_t workspace_bytes, int B, int C, int H, int W, int dtype, void *stream)
{
    if (!x || !all_set(p) || !y || !saved || !workspace) return DLKA_ERR_NULL;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return DLKA_ERR_SHAPE;
    if (!plain_supported(B, C, H, W, dtype)) return DLKA_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const LkaPlainCl G(B, C, H, W, dtype);
    Carver sv(saved, saved_bytes), cv(workspace, workspace_bytes);
    const LkaPlainSaved S = carve_plain_saved(sv, G);
    const LkaPlainFwdWs Wf = carve_plain_fwd_ws(cv, G);
    if (!sv.ok() || !cv.ok()) return DLKA_ERR_WORKSPACE;
    const float *N0 = nullptr;
    PrepPlain PW;
    DLKA_TRY(carve_prep_plain(G, S.prep, PW, p, st, true));
    DLKA_TRY(launch_cl_transpose((const float *)x, S.xt, B, C, G.pw.N, 1, st, G.bf));                                              // NCHW -> NHWC
    DLKA_TRY(dense_forward(G.pw, S.xt, N0, (const float *)p->proj_1_b, S.h, 0, PW.pw_f[0], 1, nullptr, S.a, st));                   // LKA.py:32-33 proj_1 + GELU
    DLKA_TRY(dw2d(G, S.a, PW.dw5, p->conv0_b, S.t1, 5, 1, st));                                                                    // :14 conv0
    DLKA_TRY(dw2d(G, S.t1, PW.dw7, p->conv_spatial_b, S.t2, 7, 3, st));                                                            // :15 conv_spatial
    DLKA_TRY(dense_forward(G.pw, S.t2, N0, (const float *)p->conv1_b, S.g1, 0, PW.pw_f[1], 2, S.a, S.m, st));                       // :16-18 conv1 + gate
    DLKA_TRY(dense_forward(G.pw, S.m, N0, (const float *)p->proj_2_b, Wf.yt, 0, PW.pw_f[2], 3, S.xt, nullptr, st));                 // :35-36 proj_2 + shortcut
    return launch_cl_transpose(Wf.yt, (float *)y, B, C, G.pw.N, 0, st, G.bf);
}

int dlka_lka2d_plain_attention_backward(const void *x, const dlka_lka2d_plain_params *p, const void *grad_y, const void *saved, size_t saved_bytes,
                                        void *grad_x, const dlka_lka2d_plain_grads *gr, void *workspace, size_t workspace_bytes, int B, int C, int H,
                                        int W, int dtype, void *stream)
{
    if (!x || !all_set(p) || !grad_y || !saved || !grad_x || !all_set(gr) || !workspace) return DLKA_ERR_NULL;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return DLKA_ERR_SHAPE;
    if (!plain_supported(B, C, H, W, dtype)) return DLKA_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const LkaPlainCl G(B, C, H, W, dtype);
    const int bf = G.bf;
    Carver sv(saved, saved_bytes), cv(workspace, workspace_bytes);
    const LkaPlainSaved S = carve_plain_saved(sv, G);
    const LkaPlainBwdWs Wb = carve_plain_bwd_ws(cv, G);
    if (!sv.ok() || !cv.ok()) return DLKA_ERR_WORKSPACE;
    const float *N0 = nullptr;
    PrepPlain PW;
    DLKA_TRY(carve_prep_plain(G, S.prep, PW, p, st, false));
    FinalizeBatch fb;
    memset(&fb, 0, sizeof(fb));
    DLKA_TRY(launch_cl_transpose((const float *)grad_y, Wb.gyt, B, C, G.pw.N, 1, st, bf));
    // proj_2 data gradient with the gate's backward in the epilogue: gg1 = gm * a, ga1 = gm * g1
    DLKA_TRY(dense_backward_data(G.pw, Wb.gyt, 0, N0, Wb.gg1, PW.pw_b[2], 4, S.a, st, S.g1, Wb.ga1));
    DLKA_TRY(dense_backward_data(G.pw, Wb.gg1, 0, N0, Wb.gt2, PW.pw_b[1], 0, nullptr, st));                                         // conv1
    DLKA_TRY(dw2d(G, Wb.gt2, PW.dw7_b, nullptr, Wb.gt1, 7, 3, st));                                                                // conv_spatial: flipped taps
    DLKA_TRY(dw2d_wgrad(G, S.t1, Wb.gt2, Wb.part_d7, gr->conv_spatial_w, gr->conv_spatial_b, 7, 3, st, &fb.j[fb.njobs++]));
    DLKA_TRY(dw2d(G, Wb.gt1, PW.dw5_b, nullptr, Wb.gaa, 5, 1, st));                                                                // conv0
    DLKA_TRY(dw2d_wgrad(G, S.a, Wb.gt1, Wb.part_d5, gr->conv0_w, gr->conv0_b, 5, 1, st, &fb.j[fb.njobs++]));
    // a = GELU(h) feeds the gate and conv0: gh = (ga1 + gaa) * gelu'(h)
    if (bf) DLKA_TRY(launch_gelu_bwd_sum<bf16_t>((const bf16_t *)S.h, (const bf16_t *)Wb.ga1, (const bf16_t *)Wb.gaa, (bf16_t *)Wb.gh, (long)G.E, st));
    else DLKA_TRY(launch_gelu_bwd_sum<float>(S.h, Wb.ga1, Wb.gaa, Wb.gh, (long)G.E, st));
    {
        WgradArgs jobs[3];
        fill_pw_wgrad(jobs[0], G.pw, S.m, Wb.gyt, Wb.part_p2);
        fill_pw_wgrad(jobs[1], G.pw, S.t2, Wb.gg1, Wb.part_c1);
        fill_pw_wgrad(jobs[2], G.pw, S.xt, Wb.gh, Wb.part_p1);
        float *const gws[3] = {(float *)gr->proj_2_w, (float *)gr->conv1_w, (float *)gr->proj_1_w};
        float *const gbs[3] = {(float *)gr->proj_2_b, (float *)gr->conv1_b, (float *)gr->proj_1_b};
        DLKA_TRY(launch_cl_wgrad_pw3(jobs, gws, gbs, st, &fb.j[fb.njobs]));
        fb.njobs += 3;
    }
    DLKA_TRY(launch_cl_wgrad_finalize(fb, st));
    DLKA_TRY(dense_backward_data(G.pw, Wb.gh, 0, N0, Wb.gxt, PW.pw_b[0], 3, Wb.gyt, st));                                           // gx = P1^T gh + gy
    return launch_cl_transpose(Wb.gxt, (float *)grad_x, B, C, G.pw.N, 0, st, bf);
}

// ---- the block's depthwise convs on their own: x / out / grad_out / grad_x [B][H][W][C] (float, or bf16 storage with DLKA_BF16), weight / grad_weight
// [C][1][k][k], bias / grad_bias [C] fp32; (k, dilation, padding) = (5, 1, 2) | (7, 3, 9), C a multiple of 32 ------------------------------------------
size_t dlka_dwconv2d_cl_workspace(const dlka_conv_geom *c, int dtype, int backward)
{
    Dw2dOp o;
    if (make_dw2d_op(c, dtype, o)) return 0;
    size_t n = align256((size_t)o.k * o.k * o.C * 4);
    if (backward) n += align256(cl_dw2d_part_floats(o.B, o.H, o.W, o.C, o.k) * 4);
    return n;
}

int dlka_dwconv2d_forward_cl(const void *x, const void *weight, const void *bias, void *out, void *workspace, size_t workspace_bytes,
                             const dlka_conv_geom *c, int dtype, void *stream)
{
    if (!x || !weight || !out || !workspace) return DLKA_ERR_NULL;
    Dw2dOp o;
    DLKA_TRY(make_dw2d_op(c, dtype, o));
    hipStream_t st = (hipStream_t)stream;
    Carver cv(workspace, workspace_bytes);
    float *wp = (float *)cv.take((size_t)o.k * o.k * o.C * 4);
    if (!cv.ok()) return DLKA_ERR_WORKSPACE;
    DLKA_TRY(launch_cl_dw_prep_weight((const float *)weight, wp, o.C, o.k * o.k, 0, st));
    Dw2dArgs d;
    memset(&d, 0, sizeof(d));
    d.in = (const float *)x; d.wp = wp; d.bias = (const float *)bias; d.out = (float *)out;
    d.B = o.B; d.H = o.H; d.W = o.W; d.C = o.C; d.act_bf16 = dtype == DLKA_BF16;
    return launch_cl_dw2d(d, o.k, o.dil, st);
}

int dlka_dwconv2d_backward_cl(const void *x, const void *weight, const void *grad_out, void *grad_x, void *grad_weight, void *grad_bias, void *workspace,
                              size_t workspace_bytes, const dlka_conv_geom *c, int dtype, void *stream)
{
    if (!x || !weight || !grad_out || !workspace) return DLKA_ERR_NULL;
    Dw2dOp o;
    DLKA_TRY(make_dw2d_op(c, dtype, o));
    if (grad_bias && !grad_weight) return DLKA_ERR_UNSUPPORTED;   // the bias sums ride in the weight-gradient kernel
    hipStream_t st = (hipStream_t)stream;
    Carver cv(workspace, workspace_bytes);
    float *wp = (float *)cv.take((size_t)o.k * o.k * o.C * 4);
    float *part = (float *)cv.take(cl_dw2d_part_floats(o.B, o.H, o.W, o.C, o.k) * 4);
    if (!cv.ok()) return DLKA_ERR_WORKSPACE;
    if (grad_x) {
        DLKA_TRY(launch_cl_dw_prep_weight((const float *)weight, wp, o.C, o.k * o.k, 1, st));
        Dw2dArgs d;
        memset(&d, 0, sizeof(d));
        d.in = (const float *)grad_out; d.wp = wp; d.out = (float *)grad_x;
        d.B = o.B; d.H = o.H; d.W = o.W; d.C = o.C; d.act_bf16 = dtype == DLKA_BF16;
        DLKA_TRY(launch_cl_dw2d(d, o.k, o.dil, st));
    }
    if (grad_weight) {
        Dw2dWgradArgs d;
        memset(&d, 0, sizeof(d));
        d.in = (const float *)x; d.g = (const float *)grad_out; d.part = part;
        d.B = o.B; d.H = o.H; d.W = o.W; d.C = o.C; d.act_bf16 = dtype == DLKA_BF16;
        FinalizeBatch fb;
        memset(&fb, 0, sizeof(fb));
        DLKA_TRY(launch_cl_dw2d_wgrad(d, o.k, o.dil, (float *)grad_weight, (float *)grad_bias, st, &fb.j[fb.njobs++]));
        DLKA_TRY(launch_cl_wgrad_finalize(fb, st));
    }
    return DLKA_OK;
}

}  // extern "C"
