// =========================================================================================================================
// The plain (non-deformable) 2-D LKA block (LKA_Attention, 2D/deformable_LKA/LKA.py:21-37; SpatialAttention of 2D/networks/MaxViT_LKA_Decoder.py:69-85)
// on the channels-last kernels:   y = proj_2( u * conv1( conv_spatial( conv0(u) ) ) ) + x,   u = GELU(proj_1 x).
// x / y arrive in the reference's NCHW layout; the block transposes once on the way in and once on the way out and runs entirely in [B][H][W][C]:
//   1x1 projections (+GELU / gate / residual epilogues)      capi_lka2d_frame.h, shared with the deformable block: the pointwise frame is changed THERE; here only the spatial stage and the buffers
//   depthwise 5x5 and 7x7 dilation 3, both with bias         cl_dw2d.hip (forward, data gradient on flipped taps, weight + bias gradient in partial tiles)
// Supported: fp32 and DLKA_BF16 (bf16 activations, fp32 parameters and accumulation), C / 32 in {1, 2, 3, 4, 6, 8, 12}; anything else DLKA_ERR_UNSUPPORTED.
// No float atomics anywhere in the block: two identical calls give the same bits.
// Also here: the two depthwise convs as single operators (dlka_dwconv2d_*_cl), for the tests that hold cl_dw2d.hip against a reference on its own.
// =========================================================================================================================
#include "capi_lka2d_frame.h"

using namespace dlka;

namespace dlka {

namespace {

// one depthwise conv of cl_dw2d.hip: extents, storage type, member (k, dilation) — and the launch arguments it gives, everything else zero
struct Dw2dOp { int B, H, W, C, bf, k, dil; };
template <class Args>
Args fill_dw2d(const Dw2dOp &o) { Args d; memset(&d, 0, sizeof(d)); d.B = o.B; d.H = o.H; d.W = o.W; d.C = o.C; d.act_bf16 = o.bf; return d; }

struct LkaPlainCl : Lka2dFrame {
    using Lka2dFrame::Lka2dFrame;
    Dw2dOp dw(int k, int dil) const { return {B, H, W, C, bf, k, dil}; }
    size_t prep_floats() const { return 6 * (pw_floats() + 64) + 2 * ((size_t)25 * C + 64) + 2 * ((size_t)49 * C + 64); }
    size_t part_dw(int k) const { return (cl_dw2d_part_floats(B, H, W, C, k) + 63) & ~(size_t)63; }
};

// prepared weights: the frame's pointwise convs, then the two depthwise convs (forward / flipped taps)
struct PrepPlain : FramePrep { float *dw5, *dw5_b, *dw7, *dw7_b; };

int carve_prep_plain(const LkaPlainCl &G, float *base, PrepPlain &t, const dlka_lka2d_plain_params *p, hipStream_t st, bool fill)
{
    PrepTake take{base};
    PrepBatch pb;
    memset(&pb, 0, sizeof(pb));
    carve_frame_prep(G, take, t, p, pb);
    t.dw5 = take((size_t)25 * G.C); t.dw5_b = take((size_t)25 * G.C);
    t.dw7 = take((size_t)49 * G.C); t.dw7_b = take((size_t)49 * G.C);
    if (!fill) return DLKA_OK;
    add_job(pb, p->conv0_w, t.dw5, G.C, G.C, 25, 0, 0, 3);
    add_job(pb, p->conv0_w, t.dw5_b, G.C, G.C, 25, 0, 0, 4);
    add_job(pb, p->conv_spatial_w, t.dw7, G.C, G.C, 49, 0, 0, 3);
    add_job(pb, p->conv_spatial_w, t.dw7_b, G.C, G.C, 49, 0, 0, 4);
    return launch_cl_prep_batch(pb, st);
}

// ---- the block's buffer layouts: one record and one carve function per buffer and direction (Carver, cl_host.h) ----------------------------------
struct LkaPlainSaved : FrameSaved { float *prep; };   // the frame's activation-typed tensors, then the prepared weights
LkaPlainSaved carve_plain_saved(Carver &sv, const LkaPlainCl &G)
{
    LkaPlainSaved S;
    S.carve(sv, G);
    S.prep = (float *)sv.take(G.prep_floats() * 4);
    return S;
}
struct LkaPlainFwdWs { float *yt; };
LkaPlainFwdWs carve_plain_fwd_ws(Carver &cv, const LkaPlainCl &G) { return {(float *)cv.take(G.E * G.SB)}; }
struct LkaPlainBwdWs {
    float *gyt, *gg1, *ga1, *gt2, *gt1, *gaa, *gh, *gxt;
    float *part_pw[3], *part_d7, *part_d5;   // part_pw: proj_2, conv1, proj_1
};
LkaPlainBwdWs carve_plain_bwd_ws(Carver &cv, const LkaPlainCl &G)
{
    LkaPlainBwdWs W;
    float **grad[8] = {&W.gyt, &W.gg1, &W.ga1, &W.gt2, &W.gt1, &W.gaa, &W.gh, &W.gxt};
    for (float **g : grad) *g = (float *)cv.take(G.E * G.SB);
    for (float *&part : W.part_pw) part = (float *)cv.take(G.part_pw() * 4);
    W.part_d7 = (float *)cv.take(G.part_dw(7) * 4); W.part_d5 = (float *)cv.take(G.part_dw(5) * 4);
    return W;
}

int plain_supported(int B, int C, int H, int W, int dtype)
{
    return (dtype == DLKA_F32 || dtype == DLKA_BF16) && B > 0 && H > 0 && W > 0 && frame_width_ok(C) && cl_dw2d_supported(B, H, W, C, 5, 1);
}

int dw2d(const Dw2dOp &o, const void *in, const float *wp, const void *bias, void *out, hipStream_t st)
{
    Dw2dArgs d = fill_dw2d<Dw2dArgs>(o);
    d.in = (const float *)in; d.wp = wp; d.bias = (const float *)bias; d.out = (float *)out;
    return launch_cl_dw2d(d, o.k, o.dil, st);
}

int dw2d_wgrad(const Dw2dOp &o, const void *in, const void *g, float *part, void *gw, void *gb, hipStream_t st, FinalizeJob *fold)
{
    Dw2dWgradArgs d = fill_dw2d<Dw2dWgradArgs>(o);
    d.in = (const float *)in; d.g = (const float *)g; d.part = part;
    return launch_cl_dw2d_wgrad(d, o.k, o.dil, (float *)gw, (float *)gb, st, fold);
}

// ---- the single operators ---------------------------------------------------------------------------------------------------------------------
int make_dw2d_op(const dlka_conv_geom *c, int dtype, Dw2dOp &o)
{
    if (!c) return DLKA_ERR_NULL;
    if (dtype != DLKA_F32 && dtype != DLKA_BF16) return DLKA_ERR_UNSUPPORTED;
    if (c->B <= 0 || c->C <= 0 || c->H <= 0 || c->W <= 0 || c->kh <= 0 || c->kw <= 0 || c->dh <= 0 || c->dw <= 0) return DLKA_ERR_SHAPE;
    if (c->D != 1 || c->kd != 1 || c->sd != 1 || c->dd != 1 || c->pd != 0) return DLKA_ERR_SHAPE;
    if (c->group != c->C || c->Cout != c->C || c->sh != 1 || c->sw != 1 || c->kh != c->kw || c->dh != c->dw || c->ph != c->pw) return DLKA_ERR_UNSUPPORTED;
    if (c->ph != c->dh * (c->kh - 1) / 2 || !cl_dw2d_supported(c->B, c->H, c->W, c->C, c->kh, c->dh)) return DLKA_ERR_UNSUPPORTED;
    o = {c->B, c->H, c->W, c->C, dtype == DLKA_BF16, c->kh, c->dh};
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
    const Dw2dOp d5 = G.dw(5, 1), d7 = G.dw(7, 3);
    PrepPlain PW;
    DLKA_TRY(carve_prep_plain(G, S.prep, PW, p, st, true));
    DLKA_TRY(frame_forward_head(G, PW, x, p->proj_1_b, S, nullptr, st));                                                                 // LKA.py:32-33 proj_1 + GELU
    DLKA_TRY(dw2d(d5, S.a, PW.dw5, p->conv0_b, S.t1, st));                                                                         // :14 conv0
    DLKA_TRY(dw2d(d7, S.t1, PW.dw7, p->conv_spatial_b, S.t2, st));                                                                 // :15 conv_spatial
    return frame_forward_tail(G, PW, p->conv1_b, p->proj_2_b, S, Wf.yt, y, st);                                                // :16-18 conv1 + gate, :35-36 proj_2 + shortcut
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
    Carver sv(saved, saved_bytes), cv(workspace, workspace_bytes);
    const LkaPlainSaved S = carve_plain_saved(sv, G);
    const LkaPlainBwdWs Wb = carve_plain_bwd_ws(cv, G);
    if (!sv.ok() || !cv.ok()) return DLKA_ERR_WORKSPACE;
    const Dw2dOp d5 = G.dw(5, 1), d7 = G.dw(7, 3);
    PrepPlain PW;
    DLKA_TRY(carve_prep_plain(G, S.prep, PW, p, st, false));
    FinalizeBatch fb;
    memset(&fb, 0, sizeof(fb));
    DLKA_TRY(frame_backward_head(G, PW, S, grad_y, Wb.gyt, Wb.gg1, Wb.ga1, Wb.gt2, st));
    DLKA_TRY(dw2d(d7, Wb.gt2, PW.dw7_b, nullptr, Wb.gt1, st));                                                                     // conv_spatial: flipped taps
    DLKA_TRY(dw2d_wgrad(d7, S.t1, Wb.gt2, Wb.part_d7, gr->conv_spatial_w, gr->conv_spatial_b, st, &fb.j[fb.njobs++]));
    DLKA_TRY(dw2d(d5, Wb.gt1, PW.dw5_b, nullptr, Wb.gaa, st));                                                                     // conv0
    DLKA_TRY(dw2d_wgrad(d5, S.a, Wb.gt1, Wb.part_d5, gr->conv0_w, gr->conv0_b, st, &fb.j[fb.njobs++]));
    DLKA_TRY(frame_backward_wgrads(G, S, gr, Wb.gyt, Wb.gg1, Wb.ga1, Wb.gaa, Wb.gh, Wb.part_pw, fb, st));
    return frame_backward_finish(G, PW, fb, Wb.gyt, Wb.gh, Wb.gxt, grad_x, st);
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
    return dw2d(o, x, wp, bias, out, st);
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
        DLKA_TRY(dw2d(o, grad_out, wp, nullptr, grad_x, st));
    }
    if (grad_weight) {
        FinalizeBatch fb;
        memset(&fb, 0, sizeof(fb));
        DLKA_TRY(dw2d_wgrad(o, x, grad_out, part, grad_weight, grad_bias, st, &fb.j[fb.njobs++]));
        DLKA_TRY(launch_cl_wgrad_finalize(fb, st));
    }
    return DLKA_OK;
}

}  // extern "C"
