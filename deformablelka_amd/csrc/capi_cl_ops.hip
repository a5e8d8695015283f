// C-ABI entry points of the single operators of the channels-last (NDHWC / token layout) fast path: stride-1 same-size convolutions on the matrix cores,
// register-tiled depthwise convs, the fused deformable backward, the layout transposes, and the thin exports over cl_norm.hip / planar_ops.hip.
// Everything here is fp32 unless stated; shapes the fast path does not cover return DLKA_ERR_UNSUPPORTED and the caller uses the
// general NCDHW entry points (dlka_capi.hip) instead — still HIP, never a CPU fallback.
#include "cl_host.h"

using namespace dlka;

extern "C" {

// ---- channels-last convolution ----------------------------------------------------------------------------------------
size_t dlka_conv3d_cl_workspace(const dlka_conv_geom *c, int dtype, int backward)
{
    SameConv s;
    if (dtype != DLKA_F32 || make_same_conv(c, s)) return 0;
    if (is_depthwise(s)) return 2 * align256((size_t)s.K * s.Cin * 4);
    size_t n = align256(dense_wp_floats(s) * 4);
    if (backward) n += align256(cl_wgrad_part_floats(s.M, s.K, s.Cout, s.Cin) * 4) + dense_wgrad_pad_bytes(s);   // (+ the zero-padded input copy of the padded weight gradient)
    return n;
}

int dlka_conv3d_forward_cl(const void *x, const void *weight, const void *bias, void *out, int out_planar, void *workspace,
                           size_t workspace_bytes, const dlka_conv_geom *c, int dtype, void *stream)
{
    if (!x || !weight || !out) return DLKA_ERR_NULL;
    if (dtype != DLKA_F32) return DLKA_ERR_UNSUPPORTED;
    SameConv s;
    DLKA_TRY(make_same_conv(c, s));
    hipStream_t st = (hipStream_t)stream;
    Carver cv(workspace, workspace_bytes);
    if (is_depthwise(s)) {
        if (!dw_supported(s) || out_planar) return DLKA_ERR_UNSUPPORTED;
        float *wp = (float *)cv.take((size_t)s.K * s.Cin * 4);
        if (!cv.ok()) return DLKA_ERR_WORKSPACE;
        return dw_forward(s, (const float *)x, (const float *)weight, (const float *)bias, (float *)out, wp, 0, st);
    }
    if (!dense_fwd_supported(s)) return DLKA_ERR_UNSUPPORTED;
    float *wp = (float *)cv.take(dense_wp_floats(s) * 4);
    if (!cv.ok()) return DLKA_ERR_WORKSPACE;
    return dense_forward(s, (const float *)x, (const float *)weight, (const float *)bias, (float *)out, out_planar, wp, 0, nullptr, nullptr, st);
}

int dlka_conv3d_backward_cl(const void *x, const void *weight, const void *grad_out, int grad_out_planar, void *grad_x, void *grad_weight,
                            void *grad_bias, void *workspace, size_t workspace_bytes, const dlka_conv_geom *c, int dtype, void *stream)
{
    if (!x || !weight || !grad_out) return DLKA_ERR_NULL;
    if (dtype != DLKA_F32) return DLKA_ERR_UNSUPPORTED;
    SameConv s;
    DLKA_TRY(make_same_conv(c, s));
    hipStream_t st = (hipStream_t)stream;
    Carver cv(workspace, workspace_bytes);
    if (is_depthwise(s)) {
        if (!dw_supported(s) || grad_out_planar) return DLKA_ERR_UNSUPPORTED;
        float *wp = (float *)cv.take((size_t)s.K * s.Cin * 4), *gwp = (float *)cv.take((size_t)s.K * s.Cin * 4);
        if (!cv.ok()) return DLKA_ERR_WORKSPACE;
        if (grad_x) DLKA_TRY(dw_forward(s, (const float *)grad_out, (const float *)weight, nullptr, (float *)grad_x, wp, 1, st));
        if (grad_weight) DLKA_TRY(dw_backward_weight(s, (const float *)x, (const float *)grad_out, (float *)grad_weight, (float *)grad_bias, gwp, st));
        else if (grad_bias) DLKA_TRY(launch_cl_colsum((const float *)grad_out, (float *)grad_bias, s.M, s.Cout, st));
        return DLKA_OK;
    }
    if (s.group != 1) return DLKA_ERR_UNSUPPORTED;
    float *wp = (float *)cv.take(dense_wp_floats(s) * 4);
    float *part = (float *)cv.take(cl_wgrad_part_floats(s.M, s.K, s.Cout, s.Cin) * 4);
    float *padb = (float *)cv.take_opt(dense_wgrad_pad_bytes(s), dense_wgrad_pad_bytes(s) != 0);
    if (!cv.ok()) return DLKA_ERR_WORKSPACE;
    if (grad_x) DLKA_TRY(dense_backward_data(s, (const float *)grad_out, grad_out_planar, (const float *)weight, (float *)grad_x, wp, 0, nullptr, st));
    if (grad_weight) DLKA_TRY(dense_backward_weight(s, (const float *)x, (const float *)grad_out, grad_out_planar, (float *)grad_weight, (float *)grad_bias, part, st, nullptr, 0, padb));
    else if (grad_bias) {
        if (grad_out_planar) DLKA_TRY(launch_bias_grad<float>((const float *)grad_out, (float *)grad_bias, s.B, s.Cout, s.N, st));
        else DLKA_TRY(launch_cl_colsum((const float *)grad_out, (float *)grad_bias, s.M, s.Cout, st));
    }
    return DLKA_OK;
}

// ---- channels-last deformable conv (x, out channels-last; offsets planar as in the reference) ---------------------------
size_t dlka_deform_conv3d_cl_workspace(const dlka_conv_geom *c, int dtype, int backward)
{
    SameConv s;
    if ((dtype != DLKA_F32 && dtype != DLKA_BF16) || make_same_conv(c, s)) return 0;
    size_t n = align256(dense_wp_floats(s) * 4);
    if (backward) n += align256(cl_wgrad_part_floats(s.M, s.K, s.Cout, s.Cin) * 4) + align256(deform_scratch_floats(s) * 4);
    else n += align256(deform_fwd_slab_floats(s) * 4);   // small volumes: the tap ranges' slabs (deform_forward)
    return n;
}

int dlka_deform_conv3d_forward_cl(const void *x, const void *offset, const void *weight, const void *bias, void *out, void *workspace,
                                  size_t workspace_bytes, const dlka_conv_geom *c, int dtype, void *stream)
{
    if (!x || !offset || !weight || !bias || !out) return DLKA_ERR_NULL;
    if (dtype != DLKA_F32 && dtype != DLKA_BF16) return DLKA_ERR_UNSUPPORTED;
    SameConv s;
    DLKA_TRY(make_same_conv(c, s));
    if (c->deformable_group != 1 || !deform_supported(s)) return DLKA_ERR_UNSUPPORTED;
    s.act_bf16 = dtype == DLKA_BF16;   // x / out bf16 storage; offsets, weight and bias stay fp32.  The arithmetic is the general operator's: fp32 samples, exact products on
                                       // the fp32-input MFMA, fp32 accumulation, ONE rounding at the store (the bf16 matrix cores are the fused block's trade, not this entry's)
    Carver cv(workspace, workspace_bytes);
    float *wp = (float *)cv.take(dense_wp_floats(s) * 4);
    float *slab = (float *)cv.take(deform_fwd_slab_floats(s) * 4);
    if (!cv.ok()) return DLKA_ERR_WORKSPACE;
    return deform_forward(s, (const float *)x, (const float *)offset, (const float *)weight, (const float *)bias, (float *)out, wp, (hipStream_t)stream, slab,
                          /* b16_cores */ false);
}

int dlka_deform_conv3d_backward_cl(const void *x, const void *offset, const void *weight, const void *grad_out, void *grad_x, void *grad_offset,
                                   void *grad_weight, void *grad_bias, void *workspace, size_t workspace_bytes, const dlka_conv_geom *c,
                                   int dtype, void *stream)
{
    if (!x || !offset || !weight || !grad_out) return DLKA_ERR_NULL;
    if (dtype != DLKA_F32 && dtype != DLKA_BF16) return DLKA_ERR_UNSUPPORTED;
    SameConv s;
    DLKA_TRY(make_same_conv(c, s));
    if (c->deformable_group != 1 || !deform_supported(s)) return DLKA_ERR_UNSUPPORTED;
    // DLKA_BF16: x / grad_out bf16 storage; offsets, weight and ALL FOUR gradients fp32 (grad_x is the fp32 accumulation target the token
    // block also uses; grad_offset is planar; the parameter gradients are fp32 masters)
    s.act_bf16 = dtype == DLKA_BF16;
    if (s.act_bf16 && grad_bias && !grad_weight) return DLKA_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    Carver cv(workspace, workspace_bytes);
    float *wp = (float *)cv.take(dense_wp_floats(s) * 4);
    float *part = (float *)cv.take(cl_wgrad_part_floats(s.M, s.K, s.Cout, s.Cin) * 4);
    float *scratch = (float *)cv.take(deform_scratch_floats(s) * 4);
    if (!cv.ok()) return DLKA_ERR_WORKSPACE;
    DLKA_TRY(deform_backward(s, (const float *)x, (const float *)offset, (const float *)weight, (const float *)grad_out, (float *)grad_x,
                             (float *)grad_offset, (float *)grad_weight, (float *)grad_bias, wp, part, scratch, st));
    return DLKA_OK;
}

// ---- channels-last 2-D DEPTHWISE deformable conv (cl_ddw2d.hip: the 2-D D-LKA block's conv0 / conv_spatial) on its own ------------------
// torchvision.ops.deform_conv2d(input, offset, weight, bias=None, stride 1, "same" padding, groups = C, one offset group) as the reference
// calls it (2D/deformable_LKA/deformable_LKA.py:18-30, 93-94).  x / out / grad_out / grad_x [B][H][W][C], offsets / grad_offset planar
// [B][2K][H][W] as torchvision lays them out, weight / grad_weight [C][1][kh][kw].  Lets the parity tests hold the fast-path kernels
// against the reference's own op (tests/test_ref_d3d_2d_gpu.py) without the rest of the block around them.
namespace {
int make_ddw2d(const dlka_conv_geom *c, DwArgs2d &d)
{
    if (!c) return DLKA_ERR_NULL;
    if (c->D != 1 || c->kd != 1 || c->sd != 1 || c->dd != 1 || c->pd != 0) return DLKA_ERR_SHAPE;
    if (c->B <= 0 || c->C <= 0 || c->H <= 0 || c->W <= 0 || c->kh <= 0 || c->kw <= 0 || c->dh <= 0 || c->dw <= 0) return DLKA_ERR_SHAPE;
    if (c->group != c->C || c->Cout != c->C || c->deformable_group != 1 || c->sh != 1 || c->sw != 1) return DLKA_ERR_UNSUPPORTED;
    if (dlka_conv_out_size(c->H, c->ph, c->dh, c->kh, 1) != c->H || dlka_conv_out_size(c->W, c->pw, c->dw, c->kw, 1) != c->W) return DLKA_ERR_UNSUPPORTED;
    if (!cl_ddw2d_supported(c->C)) return DLKA_ERR_UNSUPPORTED;
    memset(&d, 0, sizeof(d));
    d.B = c->B; d.H = c->H; d.W = c->W; d.C = c->C; d.kh = c->kh; d.kw = c->kw; d.ph = c->ph; d.pw = c->pw; d.dh = c->dh; d.dw = c->dw;
    return DLKA_OK;
}
}  // namespace

size_t dlka_deform_dwconv2d_cl_workspace(const dlka_conv_geom *c, int dtype, int backward)
{
    DwArgs2d d;
    if (dtype != DLKA_F32 || make_ddw2d(c, d)) return 0;
    size_t n = align256((size_t)d.kh * d.kw * d.C * 4);
    if (backward) n += align256(cl_ddw2d_part_floats(d.B * d.H * d.W, d.kh * d.kw, d.C) * 4);
    return n;
}

int dlka_deform_dwconv2d_forward_cl(const void *x, const void *offset, const void *weight, void *out, void *workspace, size_t workspace_bytes,
                                    const dlka_conv_geom *c, int dtype, void *stream)
{
    if (!x || !offset || !weight || !out) return DLKA_ERR_NULL;
    if (dtype != DLKA_F32) return DLKA_ERR_UNSUPPORTED;
    DwArgs2d d;
    DLKA_TRY(make_ddw2d(c, d));
    hipStream_t st = (hipStream_t)stream;
    Carver cv(workspace, workspace_bytes);
    float *wp = (float *)cv.take((size_t)d.kh * d.kw * d.C * 4);
    if (!cv.ok()) return DLKA_ERR_WORKSPACE;
    DLKA_TRY(launch_cl_dw_prep_weight((const float *)weight, wp, d.C, d.kh * d.kw, 0, st));
    d.in = (const float *)x; d.off = (const float *)offset; d.wp = wp; d.out = (float *)out;
    return launch_cl_ddw2d_fwd(d, st);
}

int dlka_deform_dwconv2d_backward_cl(const void *x, const void *offset, const void *weight, const void *grad_out, void *grad_x, void *grad_offset,
                                     void *grad_weight, void *workspace, size_t workspace_bytes, const dlka_conv_geom *c, int dtype, void *stream)
{
    if (!x || !offset || !weight || !grad_out || !grad_x || !grad_offset || !grad_weight) return DLKA_ERR_NULL;   // one traversal produces all three
    if (dtype != DLKA_F32) return DLKA_ERR_UNSUPPORTED;
    DwArgs2d d;
    DLKA_TRY(make_ddw2d(c, d));
    hipStream_t st = (hipStream_t)stream;
    Carver cv(workspace, workspace_bytes);
    float *wp = (float *)cv.take((size_t)d.kh * d.kw * d.C * 4);
    float *part = (float *)cv.take(cl_ddw2d_part_floats(d.B * d.H * d.W, d.kh * d.kw, d.C) * 4);
    if (!cv.ok()) return DLKA_ERR_WORKSPACE;
    DLKA_TRY(launch_cl_dw_prep_weight((const float *)weight, wp, d.C, d.kh * d.kw, 0, st));
    DLKA_TRY(launch_zero(grad_x, (size_t)d.B * d.H * d.W * d.C * 4, st));   // the window scatter accumulates with atomics
    d.in = (const float *)x; d.off = (const float *)offset; d.wp = wp; d.g = (const float *)grad_out;
    d.gx = (float *)grad_x; d.goff = (float *)grad_offset; d.part = part;
    return launch_cl_ddw2d_bwd(d, (float *)grad_weight, st);
}

// ---- layout helpers -------------------------------------------------------------------------------------------------------
int dlka_ncdhw_to_ndhwc(const void *src, void *dst, int B, int C, int N, int dtype, void *stream)
{
    if (!src || !dst) return DLKA_ERR_NULL;
    if (dtype != DLKA_F32) return DLKA_ERR_UNSUPPORTED;
    return launch_cl_transpose((const float *)src, (float *)dst, B, C, N, 1, (hipStream_t)stream);
}
int dlka_ndhwc_to_ncdhw(const void *src, void *dst, int B, int C, int N, int dtype, void *stream)
{
    if (!src || !dst) return DLKA_ERR_NULL;
    if (dtype != DLKA_F32) return DLKA_ERR_UNSUPPORTED;
    return launch_cl_transpose((const float *)src, (float *)dst, B, C, N, 0, (hipStream_t)stream);
}

// ---- the wrapper block's non-convolutional pieces (cl_norm.hip) ------------------------------------------------------------
int dlka_layernorm_tokens_forward(const void *x, int x_planar, const void *pos, const void *w, const void *b, void *xt, void *xn, void *stats, int B,
                                  int N, int C, float eps, int dtype, void *stream)
{
    if (!x || !w || !b || !xt || !xn || !stats) return DLKA_ERR_NULL;
    if (dtype != DLKA_F32) return DLKA_ERR_UNSUPPORTED;
    if (B <= 0 || N <= 0 || C <= 0) return DLKA_ERR_SHAPE;
    return launch_cl_layernorm_fwd((const float *)x, x_planar, (const float *)pos, (const float *)w, (const float *)b, (float *)xt, (float *)xn,
                                   (float *)stats, B, N, C, eps, (hipStream_t)stream);
}

int dlka_layernorm_tokens_backward(const void *g_xn, const void *g_res, const void *xt, const void *stats, const void *w, void *gxt, void *gw,
                                   void *gb, void *gpos, int B, int N, int C, int dtype, void *stream)
{
    if (!g_xn || !xt || !stats || !w || !gxt || !gw || !gb) return DLKA_ERR_NULL;
    if (dtype != DLKA_F32) return DLKA_ERR_UNSUPPORTED;
    if (B <= 0 || N <= 0 || C <= 0) return DLKA_ERR_SHAPE;
    return launch_cl_layernorm_bwd((const float *)g_xn, (const float *)g_res, (const float *)xt, (const float *)stats, (const float *)w, (float *)gxt,
                                   (float *)gw, (float *)gb, (float *)gpos, B, N, C, (hipStream_t)stream);
}

int dlka_scale_residual_forward(const void *xt, const void *e, const void *gamma, void *out, int64_t M, int C, int dtype, void *stream)
{
    if (!xt || !e || !gamma || !out) return DLKA_ERR_NULL;
    if (dtype != DLKA_F32) return DLKA_ERR_UNSUPPORTED;
    if (M <= 0 || C <= 0) return DLKA_ERR_SHAPE;
    return launch_cl_scale_residual_fwd((const float *)xt, (const float *)e, (const float *)gamma, (float *)out, (long)M, C, (hipStream_t)stream);
}

int dlka_scale_residual_backward(const void *g, const void *e, const void *gamma, void *ge, void *ggamma, int64_t M, int C, int dtype, void *stream)
{
    if (!g || !e || !gamma || !ge || !ggamma) return DLKA_ERR_NULL;
    if (dtype != DLKA_F32) return DLKA_ERR_UNSUPPORTED;
    if (M <= 0 || C <= 0 || C > 1024 || C % 32) return DLKA_ERR_SHAPE;
    return launch_cl_scale_residual_bwd((const float *)g, (const float *)e, (const float *)gamma, (float *)ge, (float *)ggamma, (long)M, C, (hipStream_t)stream);
}

int dlka_batchnorm_cl_forward(const void *x, const void *res, const void *w, const void *b, void *stats, int training, void *y, void *scratch, int64_t M,
                              int C, float eps, float slope, int dtype, void *stream)
{
    if (!x || !w || !b || !stats || !y || !scratch) return DLKA_ERR_NULL;
    if (dtype != DLKA_F32) return DLKA_ERR_UNSUPPORTED;
    if (M <= 0 || C <= 0 || C > 1024 || C % 32) return DLKA_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    if (training) DLKA_TRY(launch_cl_bn_stats((const float *)x, (float *)scratch, (float *)stats, (long)M, C, eps, st));
    return launch_cl_bn_apply((const float *)x, (const float *)res, (const float *)w, (const float *)b, (const float *)stats, nullptr, (float *)y, (long)M, (long)M, C, slope, st);
}

int dlka_batchnorm_cl_backward(const void *g, const void *x, const void *y, const void *w, const void *stats, int training, void *gx, void *gres,
                               void *gw, void *gb, void *scratch, int64_t M, int C, float slope, int dtype, void *stream)
{
    if (!g || !x || !y || !w || !stats || !gx || !gw || !gb || !scratch) return DLKA_ERR_NULL;
    if (dtype != DLKA_F32) return DLKA_ERR_UNSUPPORTED;
    if (M <= 0 || C <= 0 || C > 1024 || C % 32) return DLKA_ERR_SHAPE;
    return launch_cl_bn_bwd((const float *)g, nullptr, (const float *)x, (const float *)y, (const float *)w, (const float *)stats, (float *)scratch, (float *)gx,
                            (float *)gres, nullptr, (float *)gw, (float *)gb, (long)M, (long)M, C, slope, training, (hipStream_t)stream);
}

// ---- planar (NCDHW) plumbing of the full net (planar_ops.hip) -----------------------------------------------------------------------
int dlka_batchnorm_planar_forward(const void *x, const void *w, const void *b, void *stats, void *y, void *scratch, int B, int C, int64_t N, float eps,
                                  void *stream)
{
    if (!x || !stats || !y || !scratch) return DLKA_ERR_NULL;
    return launch_pl_bn_forward((const float *)x, (const float *)w, (const float *)b, (float *)stats, (float *)y, (float *)scratch, B, C, (long)N, eps,
                                (hipStream_t)stream);
}

int dlka_batchnorm_planar_backward(const void *g, const void *x, const void *w, const void *stats, void *gx, void *gw, void *gb, void *scratch, int B, int C,
                                   int64_t N, void *stream)
{
    if (!g || !x || !stats || !gx || !scratch) return DLKA_ERR_NULL;
    return launch_pl_bn_backward((const float *)g, (const float *)x, (const float *)w, (const float *)stats, (float *)gx, (float *)gw, (float *)gb,
                                 (float *)scratch, B, C, (long)N, (hipStream_t)stream);
}

int dlka_pointwise_planar_forward(const void *x, const void *w, const void *bias, void *y, int B, int Cin, int Cout, int64_t N, void *stream)
{
    if (!x || !w || !y) return DLKA_ERR_NULL;
    return launch_pl_pw_forward((const float *)x, (const float *)w, (const float *)bias, (float *)y, B, Cin, Cout, (long)N, (hipStream_t)stream);
}

int dlka_pointwise_planar_backward(const void *x, const void *w, const void *g, void *gx, void *gw, void *gb, int B, int Cin, int Cout, int64_t N, void *stream)
{
    if (!x || !w || !g) return DLKA_ERR_NULL;
    return launch_pl_pw_backward((const float *)x, (const float *)w, (const float *)g, (float *)gx, (float *)gw, (float *)gb, B, Cin, Cout, (long)N,
                                 (hipStream_t)stream);
}

int dlka_channel_scale(const void *x, const void *mask, void *y, int B, int64_t N, int C, int dtype, void *stream)
{
    if (!x || !mask || !y) return DLKA_ERR_NULL;
    if (dtype != DLKA_F32) return DLKA_ERR_UNSUPPORTED;
    if (B <= 0 || N <= 0 || C <= 0) return DLKA_ERR_SHAPE;
    return launch_cl_channel_scale((const float *)x, (const float *)mask, (float *)y, B, (long)N, C, (hipStream_t)stream);
}


}  // extern "C"
