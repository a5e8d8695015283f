// C-ABI entry points of libdlka_hip.so (declared in include/dlka.h): argument validation that mirrors the
// reference's AT_ASSERTM checks (3D/dcn/src/cuda/deform_conv_cuda.cu:41-76,193-200), workspace carving and the
// launch sequences.  No allocation, no synchronisation: every function is legal inside hipGraph capture.
#include <algorithm>
#include <initializer_list>

#include "cl_host.h"

using namespace dlka;

namespace {

int make_geom(const dlka_conv_geom *c, bool deform, Geom &g)
{
    if (!c) return DLKA_ERR_NULL;
    if (c->B <= 0 || c->C <= 0 || c->D <= 0 || c->H <= 0 || c->W <= 0 || c->Cout <= 0) return DLKA_ERR_SHAPE;
    if (c->kd <= 0 || c->kh <= 0 || c->kw <= 0 || c->sd <= 0 || c->sh <= 0 || c->sw <= 0) return DLKA_ERR_SHAPE;
    if (c->dd <= 0 || c->dh <= 0 || c->dw <= 0 || c->pd < 0 || c->ph < 0 || c->pw < 0) return DLKA_ERR_SHAPE;
    if (c->group <= 0 || c->C % c->group != 0 || c->Cout % c->group != 0) return DLKA_ERR_GROUP;  // cu:65-66
    g.B = c->B; g.C = c->C; g.D = c->D; g.H = c->H; g.W = c->W; g.Cout = c->Cout;
    g.kd = c->kd; g.kh = c->kh; g.kw = c->kw; g.sd = c->sd; g.sh = c->sh; g.sw = c->sw;
    g.pd = c->pd; g.ph = c->ph; g.pw = c->pw; g.dd = c->dd; g.dh = c->dh; g.dw = c->dw;
    g.group = c->group;
    g.dg = deform ? c->deformable_group : 1;
    if (deform) {
        if (g.dg <= 0 || g.C % g.dg != 0) return DLKA_ERR_DEFORM_GROUP;
        // im2col_step only exists for API parity: the reference requires batch % min(batch, step) == 0 (cu:59-63)
        if (c->im2col_step > 0) {
            const int step = c->B < c->im2col_step ? c->B : c->im2col_step;
            if (c->B % step != 0) return DLKA_ERR_IM2COL_STEP;
        } else if (c->im2col_step < 0) {
            return DLKA_ERR_IM2COL_STEP;
        }
    }
    g.Do = dlka_conv_out_size(g.D, g.pd, g.dd, g.kd, g.sd);
    g.Ho = dlka_conv_out_size(g.H, g.ph, g.dh, g.kh, g.sh);
    g.Wo = dlka_conv_out_size(g.W, g.pw, g.dw, g.kw, g.sw);
    if (g.Do <= 0 || g.Ho <= 0 || g.Wo <= 0) return DLKA_ERR_SHAPE;
    g.K = g.kd * g.kh * g.kw;
    g.Cg = g.C / g.group;
    g.Og = g.Cout / g.group;
    g.cpdg = g.C / g.dg;
    const long No = (long)g.Do * g.Ho * g.Wo, Ni = (long)g.D * g.H * g.W;
    // 32-bit plane indexing inside the kernels
    if (No > (1l << 30) || Ni > (1l << 30) || (long)g.B * g.C > (1l << 24) || (long)g.B * g.Cout > (1l << 24)) return DLKA_ERR_SHAPE;
    g.No = (int)No;
    g.Ni = (int)Ni;
    return DLKA_OK;
}

inline size_t esz(int dtype) { return dtype == DLKA_BF16 ? 2 : 4; }

// ---------------------------------------------------------------------------------------------
// typed implementations
// ---------------------------------------------------------------------------------------------
size_t deform_fwd_ws(const Geom &g) { return align256((size_t)deform_fwd_wt_floats(g) * 4); }

size_t deform_bwd_ws(const Geom &g, int dtype)
{
    size_t n = align256((size_t)deform_fwd_wt_floats(g) * 4);
    if (dtype != DLKA_F32) {
        n += align256((size_t)g.B * g.C * g.Ni * 4);          // fp32 grad_x accumulation
        n += align256((size_t)g.Cout * g.Cg * g.K * 4);       // fp32 grad_weight accumulation
    }
    return n;
}

template <typename T, int NOFF>
int deform_forward_t(const void *x, const void *off, const void *w, const void *bias, void *out, void *ws, size_t wsb,
                     const Geom &g, hipStream_t st)
{
    Carver cv(ws, wsb);
    float *wt = (float *)cv.take((size_t)deform_fwd_wt_floats(g) * 4);
    if (!cv.ok() || !wt) return DLKA_ERR_WORKSPACE;
    return launch_deform_fwd<T, NOFF>((const T *)x, (const T *)off, (const T *)w, (const T *)bias, (T *)out, wt, g, st);
}

// The backward pass of a deformable conv, written once for the operator entries and both blocks.  Every output may be null: gx || goff gates the weight
// relayout and the input / offset kernel, gw the weight part, gb the bias part (the 2-D block's depthwise deformable convs have no bias).
// wt: deform_fwd_wt_floats(g) floats for the re-laid-out weight.  grad_input and grad_weight are accumulated in fp32: in the output itself for T = float,
// else in the caller's gx32buf / gw32buf (B C Ni and Cout Cg K floats; gx32buf may be null where gx is) and cast into the output afterwards.
// (w, gw, gb: tensors of T, untyped as the parameter records of the blocks and the entry points hold them.)
template <typename T, int NOFF>
int deform_bwd_seq(const T *x, const T *off, const void *w, const T *gout, T *gx, T *goff, void *gw, void *gb, float *wt, float *gx32buf, float *gw32buf,
                   const Geom &g, hipStream_t st)
{
    constexpr bool f32 = std::is_same<T, float>::value;
    const int OgP = round_up(g.Og, deform_pick_cob(g.Og));
    const size_t nx = (size_t)g.B * g.C * g.Ni, nw = (size_t)g.Cout * g.Cg * g.K;
    float *gx32 = f32 ? (float *)gx : gx32buf, *gw32 = f32 ? (float *)gw : gw32buf;
    if (gx || goff) {
        DLKA_TRY(launch_relayout_weight<T>((const T *)w, wt, g.group, g.Og, g.Cg, g.K, OgP, st));
        if (gx32) { if (launch_zero(gx32, nx * 4, st) != DLKA_OK) return DLKA_ERR_LAUNCH; }
        DLKA_TRY((launch_deform_bwd_input_offset<T, NOFF>(x, off, wt, OgP, gout, gx32, goff, g, st)));
        if (gx && !f32) DLKA_TRY(launch_cast_from_f32<T>(gx32, gx, (long)nx, st));
    }
    if (gw) {
        if (launch_zero(gw32, nw * 4, st) != DLKA_OK) return DLKA_ERR_LAUNCH;
        DLKA_TRY((launch_deform_bwd_weight<T, NOFF>(x, off, gout, gw32, g, st)));
        if (!f32) DLKA_TRY(launch_cast_from_f32<T>(gw32, (T *)gw, (long)nw, st));
    }
    if (gb) DLKA_TRY(launch_bias_grad<T>(gout, (T *)gb, g.B, g.Cout, g.No, st));
    return DLKA_OK;
}

template <typename T, int NOFF>
int deform_backward_t(const void *x, const void *off, const void *w, const void *gout, void *gx, void *goff, void *gw,
                      void *gb, void *ws, size_t wsb, const Geom &g, hipStream_t st)
{
    Carver cv(ws, wsb);
    float *wt = (float *)cv.take((size_t)deform_fwd_wt_floats(g) * 4);
    float *gx32 = nullptr, *gw32 = nullptr;
    if (!std::is_same<T, float>::value) {   // (the areas deform_bwd_ws adds for dtype != DLKA_F32)
        if (gx) gx32 = (float *)cv.take((size_t)g.B * g.C * g.Ni * 4);
        if (gw) gw32 = (float *)cv.take((size_t)g.Cout * g.Cg * g.K * 4);
    }
    if (!cv.ok() || !wt) return DLKA_ERR_WORKSPACE;
    return deform_bwd_seq<T, NOFF>((const T *)x, (const T *)off, w, (const T *)gout, (T *)gx, (T *)goff, gw, gb, wt, gx32, gw32, g, st);
}

size_t conv_fwd_ws(const Geom &g) { return align256((size_t)conv_fwd_wt_floats(g) * 4); }
size_t conv_bwd_ws(const Geom &g, int dtype)
{
    size_t n = align256((size_t)conv_bwd_wb_floats(g) * 4);
    if (dtype != DLKA_F32) n += align256((size_t)g.Cout * g.Cg * g.K * 4);
    n += align256(conv_bwd_weight_part_floats(g, dtype == DLKA_F32 ? 4 : 2) * 4);
    return n;
}

template <typename T>
int conv_forward_t(const void *x, const void *w, const void *bias, void *out, void *ws, size_t wsb, const Geom &g, hipStream_t st)
{
    Carver cv(ws, wsb);
    float *wt = (float *)cv.take((size_t)conv_fwd_wt_floats(g) * 4);
    if (!cv.ok() || !wt) return DLKA_ERR_WORKSPACE;
    return launch_conv_fwd<T>((const T *)x, (const T *)w, (const T *)bias, (T *)out, wt, g, st);
}

// The backward pass of a plain conv, written once for the operator entry and both blocks; gx, gw and gb may each be null.  wb: conv_bwd_wb_floats(g) floats.
// grad_weight is accumulated in fp32: in gw itself for T = float, else in gw32buf (Cout Cg K floats) and cast afterwards.  part: the weight gradient's
// partial-tile buffer (conv_bwd_weight_part_floats) or null — WHICH weight-gradient kernel runs depends on it (launch_conv_bwd_weight).  w, gw, gb: as above.
template <typename T>
int conv_bwd_seq(const T *x, const void *w, const T *gout, T *gx, void *gw, void *gb, float *wb, float *gw32buf, float *part, const Geom &g, hipStream_t st)
{
    constexpr bool f32 = std::is_same<T, float>::value;
    const size_t nw = (size_t)g.Cout * g.Cg * g.K;
    if (gx) DLKA_TRY(launch_conv_bwd_data<T>(gout, (const T *)w, gx, wb, g, st));
    if (gw) {
        float *gw32 = f32 ? (float *)gw : gw32buf;
        if (launch_zero(gw32, nw * 4, st) != DLKA_OK) return DLKA_ERR_LAUNCH;
        DLKA_TRY(launch_conv_bwd_weight<T>(x, gout, gw32, g, st, part));
        if (!f32) DLKA_TRY(launch_cast_from_f32<T>(gw32, (T *)gw, (long)nw, st));
    }
    if (gb) DLKA_TRY(launch_bias_grad<T>(gout, (T *)gb, g.B, g.Cout, g.No, st));
    return DLKA_OK;
}

template <typename T>
int conv_backward_t(const void *x, const void *w, const void *gout, void *gx, void *gw, void *gb, void *ws, size_t wsb, const Geom &g, hipStream_t st)
{
    Carver cv(ws, wsb);
    float *wb = (float *)cv.take((size_t)conv_bwd_wb_floats(g) * 4);
    float *gw32 = gw && !std::is_same<T, float>::value ? (float *)cv.take((size_t)g.Cout * g.Cg * g.K * 4) : nullptr;
    const size_t npart = conv_bwd_weight_part_floats(g, sizeof(T));
    float *part = npart ? (float *)cv.take(npart * 4) : nullptr;
    if (!cv.ok() || !wb) return DLKA_ERR_WORKSPACE;
    return conv_bwd_seq<T>((const T *)x, w, (const T *)gout, (T *)gx, gw, gb, wb, gw32, part, g, st);
}

// ---- geometry builders for the fixed convs of the two blocks --------------------------------------------
Geom conv_geom(int B, int C, int Cout, int D, int H, int W, int kd, int kh, int kw, int pd, int ph, int pw, int dil_d, int dil_h,
               int dil_w, int group)
{
    dlka_conv_geom c;
    memset(&c, 0, sizeof(c));
    c.B = B; c.C = C; c.D = D; c.H = H; c.W = W; c.Cout = Cout;
    c.kd = kd; c.kh = kh; c.kw = kw; c.sd = c.sh = c.sw = 1;
    c.pd = pd; c.ph = ph; c.pw = pw; c.dd = dil_d; c.dh = dil_h; c.dw = dil_w;
    c.group = group; c.deformable_group = 1; c.im2col_step = 64;
    Geom g;
    memset(&g, 0, sizeof(g));
    make_geom(&c, true, g);
    return g;
}

// ---- sizes over the convs of a block -----------------------------------------------------------------------------------
using GeomList = std::initializer_list<const Geom *>;
// floats of the ONE scratch area every conv of a block re-lays its weight into: the largest forward / backward relayout of `convs`, and the largest
// deformable relayout of `deforms`
size_t max_relayout_floats(GeomList convs, GeomList deforms)
{
    int m = 0;
    for (const Geom *g : convs) m = std::max({m, conv_fwd_wt_floats(*g), conv_bwd_wb_floats(*g)});
    for (const Geom *g : deforms) m = std::max(m, deform_fwd_wt_floats(*g));
    return (size_t)m;
}
// elements of the largest weight tensor (the fp32 grad_weight accumulator of the bf16 path)
size_t largest_weight_elems(GeomList convs)
{
    size_t m = 0;
    for (const Geom *g : convs) m = std::max(m, (size_t)g->Cout * g->Cg * g->K);
    return m;
}

struct Lka3dGeoms {
    Geom pw, dw5, dw7, offc, dcn;
    long E, Off;
    Lka3dGeoms(int B, int C, int D, int H, int W)
    {
        pw = conv_geom(B, C, C, D, H, W, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1);
        dw5 = conv_geom(B, C, C, D, H, W, 5, 5, 5, 2, 2, 2, 1, 1, 1, C);        // transformerblock.py:637
        dw7 = conv_geom(B, C, C, D, H, W, 7, 7, 7, 9, 9, 9, 3, 3, 3, C);        // :638
        offc = conv_geom(B, C, 81, D, H, W, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1);      // synapse/deform_conv.py:80-85
        dcn = conv_geom(B, C, C, D, H, W, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1);        // transformerblock.py:639
        E = (long)B * C * D * H * W;
        Off = (long)B * 81 * D * H * W;
    }
    // the deformable relayout over dcn alone, the block's one deformable conv.  (Lka2dGeoms takes it over all five; callers size their buffers by these
    // numbers, so neither term may change.)
    size_t scratch_floats() const { return max_relayout_floats({&pw, &dw5, &dw7, &offc, &dcn}, {&dcn}); }
    size_t max_weight_elems() const { return largest_weight_elems({&pw, &dw5, &dw7, &offc, &dcn}); }
};

// ---- buffer layouts of the planar blocks (3-D and 2-D; GEOMS = Lka3dGeoms / Lka2dGeoms): one record and ONE carve function per buffer and direction ----
// `saved`: seven tensors of the block's dtype (the 2-D block's: PlanarSaved2d, behind Lka2dGeoms)
template <typename T> struct PlanarSaved { T *h, *a, *t1, *t, *off, *f, *g1; };
template <typename T>
PlanarSaved<T> carve_lka3d_saved(Carver &sv, const Lka3dGeoms &G)
{
    const size_t e = sizeof(T);
    PlanarSaved<T> S;
    S.h = (T *)sv.take(G.E * e); S.a = (T *)sv.take(G.E * e); S.t1 = (T *)sv.take(G.E * e); S.t = (T *)sv.take(G.E * e);
    S.off = (T *)sv.take(G.Off * e); S.f = (T *)sv.take(G.E * e); S.g1 = (T *)sv.take(G.E * e);
    return S;
}
// `workspace`, forward and backward call.  goff_elems: the (larger) offset tensor's size — bO holds grad_offset of one deformable conv at a time
template <typename T> struct PlanarFwdWs { float *wt; T *m; };
template <typename T> struct PlanarBwdWs { float *scr; T *bA, *bB, *bC, *bD, *bO; float *gw32, *gx32; };   // gw32, gx32: fp32 accumulators of the bf16 path
template <typename T, typename GEOMS>
PlanarFwdWs<T> carve_planar_fwd_ws(Carver &cv, const GEOMS &G)
{
    PlanarFwdWs<T> W;
    W.wt = (float *)cv.take(G.scratch_floats() * 4);
    W.m = (T *)cv.take(G.E * sizeof(T));
    return W;
}
template <typename T, typename GEOMS>
PlanarBwdWs<T> carve_planar_bwd_ws(Carver &cv, const GEOMS &G, size_t goff_elems, int dtype)
{
    const size_t e = sizeof(T);
    PlanarBwdWs<T> W;
    W.scr = (float *)cv.take(G.scratch_floats() * 4);
    W.bA = (T *)cv.take(G.E * e); W.bB = (T *)cv.take(G.E * e); W.bC = (T *)cv.take(G.E * e); W.bD = (T *)cv.take(G.E * e);
    W.bO = (T *)cv.take(goff_elems * e);
    W.gw32 = dtype != DLKA_F32 ? (float *)cv.take(G.max_weight_elems() * 4) : nullptr;
    W.gx32 = dtype != DLKA_F32 ? (float *)cv.take(G.E * 4) : nullptr;
    return W;
}
template <typename T, typename GEOMS>
size_t planar_workspace_bytes(const GEOMS &G, size_t goff_elems, int dtype)
{
    const size_t f = carved_bytes([&](Carver &m) { carve_planar_fwd_ws<T>(m, G); });
    const size_t b = carved_bytes([&](Carver &m) { carve_planar_bwd_ws<T>(m, G, goff_elems, dtype); });
    return f > b ? f : b;
}

template <typename T>
int lka3d_forward_t(const void *x, const dlka_lka3d_params *p, void *y, void *saved, size_t savedb, void *ws, size_t wsb,
                    int B, int C, int D, int H, int W, hipStream_t st)
{
    Lka3dGeoms G(B, C, D, H, W);
    Carver sv(saved, savedb), cv(ws, wsb);
    const PlanarSaved<T> S = carve_lka3d_saved<T>(sv, G);
    const PlanarFwdWs<T> Wf = carve_planar_fwd_ws<T>(cv, G);
    if (!sv.ok() || !cv.ok()) return DLKA_ERR_WORKSPACE;
    T *h = S.h, *a = S.a, *t1 = S.t1, *t = S.t, *off = S.off, *f = S.f, *g1 = S.g1, *m = Wf.m;
    float *wt = Wf.wt;
    DLKA_TRY(launch_conv_fwd<T>((const T *)x, (const T *)p->proj_1_w, (const T *)p->proj_1_b, h, wt, G.pw, st));          // :667
    DLKA_TRY(launch_gelu_fwd<T>(h, a, G.E, st));                                                                          // :668
    DLKA_TRY(launch_conv_fwd<T>(a, (const T *)p->conv0_w, (const T *)p->conv0_b, t1, wt, G.dw5, st));                     // :646
    DLKA_TRY(launch_conv_fwd<T>(t1, (const T *)p->conv_spatial_w, (const T *)p->conv_spatial_b, t, wt, G.dw7, st));       // :647
    DLKA_TRY(launch_conv_fwd<T>(t, (const T *)p->offset_w, (const T *)p->offset_b, off, wt, G.offc, st));                 // deform_conv.py:94
    DLKA_TRY((launch_deform_fwd<T, 3>(t, off, (const T *)p->deform_w, (const T *)p->deform_b, f, wt, G.dcn, st)));        // deform_conv.py:95-105
    DLKA_TRY(launch_conv_fwd<T>(f, (const T *)p->conv1_w, (const T *)p->conv1_b, g1, wt, G.pw, st));                      // :650
    DLKA_TRY(launch_mul_fwd<T>(a, g1, m, G.E, st));                                                                       // :652
    DLKA_TRY(launch_conv_fwd<T>(m, (const T *)p->proj_2_w, (const T *)p->proj_2_b, (T *)y, wt, G.pw, st));                // :670
    DLKA_TRY(launch_add_fwd<T>((const T *)y, (const T *)x, (T *)y, G.E, st));                                             // :671
    return DLKA_OK;
}

template <typename T>
int lka3d_backward_t(const void *x_, const dlka_lka3d_params *p, const void *gy_, const void *saved, size_t savedb, void *gx_,
                     const dlka_lka3d_grads *gr, void *ws, size_t wsb, int B, int C, int D, int H, int W, int dtype, hipStream_t st)
{
    Lka3dGeoms G(B, C, D, H, W);
    Carver sv(saved, savedb), cv(ws, wsb);
    const PlanarSaved<T> S = carve_lka3d_saved<T>(sv, G);
    const PlanarBwdWs<T> Wb = carve_planar_bwd_ws<T>(cv, G, G.Off, dtype);
    if (!sv.ok() || !cv.ok()) return DLKA_ERR_WORKSPACE;
    const T *h = S.h, *a = S.a, *t1 = S.t1, *t = S.t, *off = S.off, *f = S.f, *g1 = S.g1;
    T *bA = Wb.bA, *bB = Wb.bB, *bC = Wb.bC, *bD = Wb.bD, *bO = Wb.bO;
    float *scr = Wb.scr, *gw32 = Wb.gw32, *gx32 = Wb.gx32;
    const T *x = (const T *)x_, *gy = (const T *)gy_;
    T *gx = (T *)gx_;

    // conv_bwd_seq's `nullptr` below: the blocks carve no partial-tile buffer, so the weight gradients take the kernels that need none
    // proj_2 (+ residual: d(x + ...)/dx adds gy at the very end)                           transformerblock.py:670-671
    DLKA_TRY(launch_mul_fwd<T>(a, g1, bA, G.E, st));                                        // m = a * g1 (recomputed)
    DLKA_TRY(conv_bwd_seq<T>(bA, p->proj_2_w, gy, bB, gr->proj_2_w, gr->proj_2_b, scr, gw32, nullptr, G.pw, st));  // bB = gm
    // gate u * attn                                                                        :652
    DLKA_TRY(launch_mul_bwd<T>(a, g1, bB, bC, bD, G.E, st));                                // bC = ga1 = gm*g1 ; bD = gg1 = gm*a
    // conv1                                                                                :650
    DLKA_TRY(conv_bwd_seq<T>(f, p->conv1_w, bD, bB, gr->conv1_w, gr->conv1_b, scr, gw32, nullptr, G.pw, st));      // bB = gf
    // deformable conv                                                                      deform_conv.py:95-105
    DLKA_TRY((deform_bwd_seq<T, 3>(t, off, p->deform_w, bB, bA, bO, gr->deform_w, gr->deform_b, scr, gx32, gw32, G.dcn, st)));  // bA = gt_a, bO = goff
    // offset-predict conv                                                                  deform_conv.py:94
    DLKA_TRY(conv_bwd_seq<T>(t, p->offset_w, bO, bD, gr->offset_w, gr->offset_b, scr, gw32, nullptr, G.offc, st)); // bD = gt_b
    DLKA_TRY(launch_add_fwd<T>(bA, bD, bA, G.E, st));                                       // bA = gt
    // depthwise 7^3 dil 3                                                                  :647
    DLKA_TRY(conv_bwd_seq<T>(t1, p->conv_spatial_w, bA, bB, gr->conv_spatial_w, gr->conv_spatial_b, scr, gw32, nullptr, G.dw7, st));  // bB = gt1
    // depthwise 5^3                                                                        :646
    DLKA_TRY(conv_bwd_seq<T>(a, p->conv0_w, bB, bD, gr->conv0_w, gr->conv0_b, scr, gw32, nullptr, G.dw5, st));     // bD = ga2
    DLKA_TRY(launch_add_fwd<T>(bC, bD, bC, G.E, st));                                       // bC = ga
    // GELU                                                                                 :668
    DLKA_TRY(launch_gelu_bwd<T>(h, bC, bA, G.E, st));                                       // bA = gh
    // proj_1                                                                               :667
    DLKA_TRY(conv_bwd_seq<T>(x, p->proj_1_w, bA, bB, gr->proj_1_w, gr->proj_1_b, scr, gw32, nullptr, G.pw, st));   // bB = gx1
    DLKA_TRY(launch_add_fwd<T>(bB, gy, gx, G.E, st));                                       // + shortcut
    return DLKA_OK;
}

// ---- 2-D block ---------------------------------------------------------------------------------------------
struct Lka2dGeoms {
    Geom pw, off5, dcn5, off7, dcn7;
    long E, Off5, Off7;
    Lka2dGeoms(int B, int C, int H, int W)
    {
        pw = conv_geom(B, C, C, 1, H, W, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1);
        off5 = conv_geom(B, C, 50, 1, H, W, 1, 5, 5, 0, 2, 2, 1, 1, 1, 1);     // deformable_LKA.py:10-16 via :93
        dcn5 = conv_geom(B, C, C, 1, H, W, 1, 5, 5, 0, 2, 2, 1, 1, 1, C);      // :18-25 via :93
        off7 = conv_geom(B, C, 98, 1, H, W, 1, 7, 7, 0, 9, 9, 1, 3, 3, 1);     // :94
        dcn7 = conv_geom(B, C, C, 1, H, W, 1, 7, 7, 0, 9, 9, 1, 3, 3, C);      // :94
        E = (long)B * C * H * W;
        Off5 = (long)B * 50 * H * W;
        Off7 = (long)B * 98 * H * W;
    }
    // the deformable relayout over ALL five, the three plain convs included: more than dcn5 and dcn7 need, and unlike Lka3dGeoms — see there
    size_t scratch_floats() const { return max_relayout_floats({&pw, &off5, &dcn5, &off7, &dcn7}, {&pw, &off5, &dcn5, &off7, &dcn7}); }
    size_t max_weight_elems() const { return largest_weight_elems({&pw, &off5, &dcn5, &off7, &dcn7}); }
};

template <typename T> struct PlanarSaved2d { T *h, *a, *o5, *t1, *o7, *t2, *g1; };
template <typename T>
PlanarSaved2d<T> carve_lka2d_saved(Carver &sv, const Lka2dGeoms &G)
{
    const size_t e = sizeof(T);
    PlanarSaved2d<T> S;
    S.h = (T *)sv.take(G.E * e); S.a = (T *)sv.take(G.E * e); S.o5 = (T *)sv.take(G.Off5 * e); S.t1 = (T *)sv.take(G.E * e);
    S.o7 = (T *)sv.take(G.Off7 * e); S.t2 = (T *)sv.take(G.E * e); S.g1 = (T *)sv.take(G.E * e);
    return S;
}
template <typename T>
int lka2d_forward_t(const void *x, const dlka_lka2d_params *p, void *y, void *saved, size_t savedb, void *ws, size_t wsb,
                    int B, int C, int H, int W, hipStream_t st)
{
    Lka2dGeoms G(B, C, H, W);
    Carver sv(saved, savedb), cv(ws, wsb);
    const PlanarSaved2d<T> S = carve_lka2d_saved<T>(sv, G);
    const PlanarFwdWs<T> Wf = carve_planar_fwd_ws<T>(cv, G);
    if (!sv.ok() || !cv.ok()) return DLKA_ERR_WORKSPACE;
    T *h = S.h, *a = S.a, *o5 = S.o5, *t1 = S.t1, *o7 = S.o7, *t2 = S.t2, *g1 = S.g1, *m = Wf.m;
    float *wt = Wf.wt;
    DLKA_TRY(launch_conv_fwd<T>((const T *)x, (const T *)p->proj_1_w, (const T *)p->proj_1_b, h, wt, G.pw, st));                     // :135
    DLKA_TRY(launch_gelu_fwd<T>(h, a, G.E, st));                                                                                     // :136
    DLKA_TRY(launch_conv_fwd<T>(a, (const T *)p->conv0_offset_w, (const T *)p->conv0_offset_b, o5, wt, G.off5, st));                 // :28
    DLKA_TRY((launch_deform_fwd<T, 2>(a, o5, (const T *)p->conv0_w, (const T *)nullptr, t1, wt, G.dcn5, st)));                       // :29
    DLKA_TRY(launch_conv_fwd<T>(t1, (const T *)p->conv_spatial_offset_w, (const T *)p->conv_spatial_offset_b, o7, wt, G.off7, st));  // :28
    DLKA_TRY((launch_deform_fwd<T, 2>(t1, o7, (const T *)p->conv_spatial_w, (const T *)nullptr, t2, wt, G.dcn7, st)));               // :29
    DLKA_TRY(launch_conv_fwd<T>(t2, (const T *)p->conv1_w, (const T *)p->conv1_b, g1, wt, G.pw, st));                                // :102
    DLKA_TRY(launch_mul_fwd<T>(a, g1, m, G.E, st));                                                                                  // :104
    DLKA_TRY(launch_conv_fwd<T>(m, (const T *)p->proj_2_w, (const T *)p->proj_2_b, (T *)y, wt, G.pw, st));                           // :138
    DLKA_TRY(launch_add_fwd<T>((const T *)y, (const T *)x, (T *)y, G.E, st));                                                        // :139
    return DLKA_OK;
}

template <typename T>
int lka2d_backward_t(const void *x_, const dlka_lka2d_params *p, const void *gy_, const void *saved, size_t savedb, void *gx_,
                     const dlka_lka2d_grads *gr, void *ws, size_t wsb, int B, int C, int H, int W, int dtype, hipStream_t st)
{
    Lka2dGeoms G(B, C, H, W);
    Carver sv(saved, savedb), cv(ws, wsb);
    const PlanarSaved2d<T> S = carve_lka2d_saved<T>(sv, G);
    const PlanarBwdWs<T> Wb = carve_planar_bwd_ws<T>(cv, G, G.Off7, dtype);
    if (!sv.ok() || !cv.ok()) return DLKA_ERR_WORKSPACE;
    const T *h = S.h, *a = S.a, *o5 = S.o5, *t1 = S.t1, *o7 = S.o7, *t2 = S.t2, *g1 = S.g1;
    T *bA = Wb.bA, *bB = Wb.bB, *bC = Wb.bC, *bD = Wb.bD, *bO = Wb.bO;
    float *scr = Wb.scr, *gw32 = Wb.gw32, *gx32 = Wb.gx32;
    const T *x = (const T *)x_, *gy = (const T *)gy_;
    T *gx = (T *)gx_;
    // (conv_bwd_seq's `nullptr`: no partial-tile buffer, as in lka3d_backward_t)
    DLKA_TRY(launch_mul_fwd<T>(a, g1, bA, G.E, st));                                                                        // m
    DLKA_TRY(conv_bwd_seq<T>(bA, p->proj_2_w, gy, bB, gr->proj_2_w, gr->proj_2_b, scr, gw32, nullptr, G.pw, st));  // bB = gm
    DLKA_TRY(launch_mul_bwd<T>(a, g1, bB, bC, bD, G.E, st));                                                                // bC = ga1, bD = gg1
    DLKA_TRY(conv_bwd_seq<T>(t2, p->conv1_w, bD, bB, gr->conv1_w, gr->conv1_b, scr, gw32, nullptr, G.pw, st));     // bB = gt2
    // conv_spatial: t2 = dcn7(t1, o7 = off7(t1))
    DLKA_TRY((deform_bwd_seq<T, 2>(t1, o7, p->conv_spatial_w, bB, bA, bO, gr->conv_spatial_w, nullptr, scr, gx32, gw32, G.dcn7, st)));  // bA = gt1_a, bO = go7
    DLKA_TRY(conv_bwd_seq<T>(t1, p->conv_spatial_offset_w, bO, bD, gr->conv_spatial_offset_w, gr->conv_spatial_offset_b, scr, gw32, nullptr, G.off7, st));  // bD = gt1_b
    DLKA_TRY(launch_add_fwd<T>(bA, bD, bA, G.E, st));                                                                       // bA = gt1
    // conv0: t1 = dcn5(a, o5 = off5(a))
    DLKA_TRY((deform_bwd_seq<T, 2>(a, o5, p->conv0_w, bA, bB, bO, gr->conv0_w, nullptr, scr, gx32, gw32, G.dcn5, st)));  // bB = ga2_a, bO = go5
    DLKA_TRY(conv_bwd_seq<T>(a, p->conv0_offset_w, bO, bD, gr->conv0_offset_w, gr->conv0_offset_b, scr, gw32, nullptr, G.off5, st));  // bD = ga2_b
    DLKA_TRY(launch_add_fwd<T>(bB, bD, bB, G.E, st));
    DLKA_TRY(launch_add_fwd<T>(bC, bB, bC, G.E, st));                                                                       // bC = ga
    DLKA_TRY(launch_gelu_bwd<T>(h, bC, bA, G.E, st));                                                                       // bA = gh
    DLKA_TRY(conv_bwd_seq<T>(x, p->proj_1_w, bA, bB, gr->proj_1_w, gr->proj_1_b, scr, gw32, nullptr, G.pw, st));   // bB = gx1
    DLKA_TRY(launch_add_fwd<T>(bB, gy, gx, G.E, st));
    return DLKA_OK;
}

#define DLKA_DISPATCH(dtype, CALL_F32, CALL_BF16) \
    ((dtype) == DLKA_F32 ? (CALL_F32) : (dtype) == DLKA_BF16 ? (CALL_BF16) : DLKA_ERR_DTYPE)

// ---- deformable conv, 3-D (NOFF = 3) and 2-D (NOFF = 2: torchvision semantics on a D = 1 geometry) ------------------------------------------
int check_2d(const dlka_conv_geom *c)
{
    if (!c) return DLKA_ERR_NULL;
    if (c->D != 1 || c->kd != 1 || c->sd != 1 || c->dd != 1 || c->pd != 0) return DLKA_ERR_SHAPE;
    return DLKA_OK;
}

// the geometry step of every deformable entry: the 2-D ones first require a flat geometry
template <int NOFF>
int deform_geom(const dlka_conv_geom *c, Geom &g)
{
    if (NOFF == 2) DLKA_TRY(check_2d(c));
    return make_geom(c, true, g);
}

template <int NOFF>
size_t deform_workspace(const dlka_conv_geom *c, int dtype, bool backward)
{
    Geom g;
    if (deform_geom<NOFF>(c, g)) return 0;
    return backward ? deform_bwd_ws(g, dtype) : deform_fwd_ws(g);
}

// (bias: required by the 3-D entry, optional in the 2-D one — checked there)
template <int NOFF>
int deform_forward(const void *x, const void *offset, const void *weight, const void *bias, void *out, void *ws, size_t wsb, const dlka_conv_geom *c,
                   int dtype, void *stream)
{
    if (!x || !offset || !weight || !out) return DLKA_ERR_NULL;
    Geom g;
    DLKA_TRY(deform_geom<NOFF>(c, g));
    hipStream_t st = (hipStream_t)stream;
    if (dtype == DLKA_F64) return launch_deform_fwd_f64<NOFF>((const double *)x, (const double *)offset, (const double *)weight, (const double *)bias, (double *)out, g, st);
    return DLKA_DISPATCH(dtype, (deform_forward_t<float, NOFF>(x, offset, weight, bias, out, ws, wsb, g, st)),
                         (deform_forward_t<bf16_t, NOFF>(x, offset, weight, bias, out, ws, wsb, g, st)));
}

template <int NOFF>
int deform_backward(const void *x, const void *offset, const void *weight, const void *gout, void *gx, void *goff, void *gw, void *gb, void *ws, size_t wsb,
                    const dlka_conv_geom *c, int dtype, void *stream)
{
    if (!x || !offset || !weight || !gout) return DLKA_ERR_NULL;
    Geom g;
    DLKA_TRY(deform_geom<NOFF>(c, g));
    hipStream_t st = (hipStream_t)stream;
    if (dtype == DLKA_F64)
        return launch_deform_bwd_f64<NOFF>((const double *)x, (const double *)offset, (const double *)weight, (const double *)gout, (double *)gx, (double *)goff,
                                           (double *)gw, (double *)gb, g, st);
    return DLKA_DISPATCH(dtype, (deform_backward_t<float, NOFF>(x, offset, weight, gout, gx, goff, gw, gb, ws, wsb, g, st)),
                         (deform_backward_t<bf16_t, NOFF>(x, offset, weight, gout, gx, goff, gw, gb, ws, wsb, g, st)));
}

template <int NOFF>
int deform_sample_index(const void *offset, int32_t *idx, uint8_t *mask, const dlka_conv_geom *c, int dtype, int path, void *stream)
{
    if (!offset || !idx || !mask) return DLKA_ERR_NULL;
    Geom g;
    DLKA_TRY(deform_geom<NOFF>(c, g));
    hipStream_t st = (hipStream_t)stream;
    if (NOFF == 2)
        return DLKA_DISPATCH(dtype, launch_sample_index2<float>((const float *)offset, idx, mask, g, path, st),
                             launch_sample_index2<bf16_t>((const bf16_t *)offset, idx, mask, g, path, st));
    return DLKA_DISPATCH(dtype, launch_sample_index<float>((const float *)offset, idx, mask, g, path, st),
                         launch_sample_index<bf16_t>((const bf16_t *)offset, idx, mask, g, path, st));
}

}  // namespace

// =================================================================================================================
// extern "C"
// =================================================================================================================
extern "C" {

int dlka_abi_version(void) { return DLKA_ABI_VERSION; }

const char *dlka_status_string(int s)
{
    switch (s) {
        case DLKA_OK: return "ok";
        case DLKA_ERR_NULL: return "null pointer argument";
        case DLKA_ERR_GROUP: return "channels and channels_out must be divisible by group";
        case DLKA_ERR_DEFORM_GROUP: return "channels must be divisible by deformable_group";
        case DLKA_ERR_SHAPE: return "invalid shape: non-positive or too large size / empty output";
        case DLKA_ERR_IM2COL_STEP: return "batch must be divisible by min(batch, im2col_step)";
        case DLKA_ERR_DTYPE: return "unsupported dtype";
        case DLKA_ERR_WORKSPACE: return "workspace / saved buffer missing or too small";
        case DLKA_ERR_UNSUPPORTED: return "unsupported parameter combination";
        case DLKA_ERR_LAUNCH: return "HIP kernel launch failed";
        default: return "unknown dlka status";
    }
}

int dlka_conv_out_size(int in, int pad, int dil, int k, int stride)
{
    if (stride <= 0) return 0;
    const int num = in + 2 * pad - (dil * (k - 1) + 1);
    if (num < 0) return 0;
    return num / stride + 1;
}

// ---- deformable conv: 3-D and 2-D entries over the same templates -----------------------------------------------------------------------------
size_t dlka_deform_conv3d_forward_workspace(const dlka_conv_geom *c, int dtype) { return deform_workspace<3>(c, dtype, false); }
size_t dlka_deform_conv3d_backward_workspace(const dlka_conv_geom *c, int dtype) { return deform_workspace<3>(c, dtype, true); }
size_t dlka_deform_conv2d_forward_workspace(const dlka_conv_geom *c, int dtype) { return deform_workspace<2>(c, dtype, false); }
size_t dlka_deform_conv2d_backward_workspace(const dlka_conv_geom *c, int dtype) { return deform_workspace<2>(c, dtype, true); }

int dlka_deform_conv3d_forward(const void *x, const void *offset, const void *weight, const void *bias, void *out,
                               void *workspace, size_t workspace_bytes, const dlka_conv_geom *c, int dtype, void *stream)
{
    if (!bias) return DLKA_ERR_NULL;
    return deform_forward<3>(x, offset, weight, bias, out, workspace, workspace_bytes, c, dtype, stream);
}

int dlka_deform_conv2d_forward(const void *x, const void *offset, const void *weight, const void *bias, void *out,
                               void *workspace, size_t workspace_bytes, const dlka_conv_geom *c, int dtype, void *stream)
{
    return deform_forward<2>(x, offset, weight, bias, out, workspace, workspace_bytes, c, dtype, stream);
}

int dlka_deform_conv3d_backward(const void *x, const void *offset, const void *weight, const void *grad_out, void *grad_x,
                                void *grad_offset, void *grad_weight, void *grad_bias, void *workspace, size_t workspace_bytes,
                                const dlka_conv_geom *c, int dtype, void *stream)
{
    return deform_backward<3>(x, offset, weight, grad_out, grad_x, grad_offset, grad_weight, grad_bias, workspace, workspace_bytes, c, dtype, stream);
}

int dlka_deform_conv2d_backward(const void *x, const void *offset, const void *weight, const void *grad_out, void *grad_x,
                                void *grad_offset, void *grad_weight, void *grad_bias, void *workspace, size_t workspace_bytes,
                                const dlka_conv_geom *c, int dtype, void *stream)
{
    return deform_backward<2>(x, offset, weight, grad_out, grad_x, grad_offset, grad_weight, grad_bias, workspace, workspace_bytes, c, dtype, stream);
}

int dlka_deform_conv3d_sample_index_path(const void *offset, int32_t *idx, uint8_t *mask, const dlka_conv_geom *c, int dtype, int path, void *stream)
{
    return deform_sample_index<3>(offset, idx, mask, c, dtype, path, stream);
}

int dlka_deform_conv3d_sample_index(const void *offset, int32_t *idx, uint8_t *mask, const dlka_conv_geom *c, int dtype, void *stream)
{
    return deform_sample_index<3>(offset, idx, mask, c, dtype, 0, stream);
}

int dlka_deform_conv2d_sample_index_path(const void *offset, int32_t *idx, uint8_t *mask, const dlka_conv_geom *c, int dtype, int path, void *stream)
{
    return deform_sample_index<2>(offset, idx, mask, c, dtype, path, stream);
}

// ---- plain conv -----------------------------------------------------------------------------------------------
size_t dlka_conv3d_forward_workspace(const dlka_conv_geom *c, int dtype)
{
    (void)dtype;
    Geom g;
    if (make_geom(c, false, g)) return 0;
    return conv_fwd_ws(g);
}

int dlka_conv3d_forward(const void *x, const void *weight, const void *bias, void *out, void *workspace, size_t workspace_bytes,
                        const dlka_conv_geom *c, int dtype, void *stream)
{
    if (!x || !weight || !out) return DLKA_ERR_NULL;
    Geom g;
    DLKA_TRY(make_geom(c, false, g));
    hipStream_t st = (hipStream_t)stream;
    if (dtype == DLKA_F64) return launch_conv_fwd_f64((const double *)x, (const double *)weight, (const double *)bias, (double *)out, g, st);
    return DLKA_DISPATCH(dtype, conv_forward_t<float>(x, weight, bias, out, workspace, workspace_bytes, g, st),
                         conv_forward_t<bf16_t>(x, weight, bias, out, workspace, workspace_bytes, g, st));
}

size_t dlka_conv3d_backward_workspace(const dlka_conv_geom *c, int dtype)
{
    Geom g;
    if (make_geom(c, false, g)) return 0;
    return conv_bwd_ws(g, dtype);
}

int dlka_conv3d_backward(const void *x, const void *weight, const void *grad_out, void *grad_x, void *grad_weight, void *grad_bias,
                         void *workspace, size_t workspace_bytes, const dlka_conv_geom *c, int dtype, void *stream)
{
    if (!x || !weight || !grad_out) return DLKA_ERR_NULL;
    Geom g;
    DLKA_TRY(make_geom(c, false, g));
    hipStream_t st = (hipStream_t)stream;
    if (dtype == DLKA_F64)
        return launch_conv_bwd_f64((const double *)x, (const double *)weight, (const double *)grad_out, (double *)grad_x, (double *)grad_weight, (double *)grad_bias, g, st);
    return DLKA_DISPATCH(dtype, conv_backward_t<float>(x, weight, grad_out, grad_x, grad_weight, grad_bias, workspace, workspace_bytes, g, st),
                         conv_backward_t<bf16_t>(x, weight, grad_out, grad_x, grad_weight, grad_bias, workspace, workspace_bytes, g, st));
}

// ---- elementwise ----------------------------------------------------------------------------------------------
int dlka_gelu_forward(const void *x, void *y, int64_t n, int dtype, void *stream)
{
    if (!x || !y) return DLKA_ERR_NULL;
    hipStream_t st = (hipStream_t)stream;
    return DLKA_DISPATCH(dtype, launch_gelu_fwd<float>((const float *)x, (float *)y, (long)n, st),
                         launch_gelu_fwd<bf16_t>((const bf16_t *)x, (bf16_t *)y, (long)n, st));
}
int dlka_gelu_backward(const void *x, const void *gy, void *gx, int64_t n, int dtype, void *stream)
{
    if (!x || !gy || !gx) return DLKA_ERR_NULL;
    hipStream_t st = (hipStream_t)stream;
    return DLKA_DISPATCH(dtype, launch_gelu_bwd<float>((const float *)x, (const float *)gy, (float *)gx, (long)n, st),
                         launch_gelu_bwd<bf16_t>((const bf16_t *)x, (const bf16_t *)gy, (bf16_t *)gx, (long)n, st));
}
int dlka_mul_forward(const void *a, const void *b, void *y, int64_t n, int dtype, void *stream)
{
    if (!a || !b || !y) return DLKA_ERR_NULL;
    hipStream_t st = (hipStream_t)stream;
    return DLKA_DISPATCH(dtype, launch_mul_fwd<float>((const float *)a, (const float *)b, (float *)y, (long)n, st),
                         launch_mul_fwd<bf16_t>((const bf16_t *)a, (const bf16_t *)b, (bf16_t *)y, (long)n, st));
}
int dlka_mul_backward(const void *a, const void *b, const void *gy, void *ga, void *gb, int64_t n, int dtype, void *stream)
{
    if (!a || !b || !gy) return DLKA_ERR_NULL;
    hipStream_t st = (hipStream_t)stream;
    return DLKA_DISPATCH(dtype, launch_mul_bwd<float>((const float *)a, (const float *)b, (const float *)gy, (float *)ga, (float *)gb, (long)n, st),
                         launch_mul_bwd<bf16_t>((const bf16_t *)a, (const bf16_t *)b, (const bf16_t *)gy, (bf16_t *)ga, (bf16_t *)gb, (long)n, st));
}
int dlka_add_forward(const void *a, const void *b, void *y, int64_t n, int dtype, void *stream)
{
    if (!a || !b || !y) return DLKA_ERR_NULL;
    hipStream_t st = (hipStream_t)stream;
    return DLKA_DISPATCH(dtype, launch_add_fwd<float>((const float *)a, (const float *)b, (float *)y, (long)n, st),
                         launch_add_fwd<bf16_t>((const bf16_t *)a, (const bf16_t *)b, (bf16_t *)y, (long)n, st));
}

// ---- blocks -----------------------------------------------------------------------------------------------------
static int check_block(int B, int C, int D, int H, int W)
{
    if (B <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0) return DLKA_ERR_SHAPE;
    if ((long)D * H * W > (1l << 30) || (long)B * (C > 98 ? C : 98) > (1l << 24)) return DLKA_ERR_SHAPE;
    return DLKA_OK;
}

size_t dlka_lka3d_saved_bytes(int B, int C, int D, int H, int W, int dtype)
{
    if (check_block(B, C, D, H, W)) return 0;
    Lka3dGeoms G(B, C, D, H, W);
    return carved_bytes([&](Carver &m) { esz(dtype) == 2 ? (void)carve_lka3d_saved<bf16_t>(m, G) : (void)carve_lka3d_saved<float>(m, G); });
}

size_t dlka_lka3d_workspace_bytes(int B, int C, int D, int H, int W, int dtype)
{
    if (check_block(B, C, D, H, W)) return 0;
    Lka3dGeoms G(B, C, D, H, W);
    return esz(dtype) == 2 ? planar_workspace_bytes<bf16_t>(G, G.Off, dtype) : planar_workspace_bytes<float>(G, G.Off, dtype);
}

int dlka_lka3d_attention_forward(const void *x, const dlka_lka3d_params *p, void *y, void *saved, size_t saved_bytes,
                                 void *workspace, size_t workspace_bytes, int B, int C, int D, int H, int W, int dtype, void *stream)
{
    if (!x || !all_set(p) || !y || !saved || !workspace) return DLKA_ERR_NULL;
    DLKA_TRY(check_block(B, C, D, H, W));
    hipStream_t st = (hipStream_t)stream;
    return DLKA_DISPATCH(dtype, lka3d_forward_t<float>(x, p, y, saved, saved_bytes, workspace, workspace_bytes, B, C, D, H, W, st),
                         lka3d_forward_t<bf16_t>(x, p, y, saved, saved_bytes, workspace, workspace_bytes, B, C, D, H, W, st));
}

int dlka_lka3d_attention_backward(const void *x, const dlka_lka3d_params *p, const void *grad_y, const void *saved, size_t saved_bytes,
                                  void *grad_x, const dlka_lka3d_grads *grads, void *workspace, size_t workspace_bytes,
                                  int B, int C, int D, int H, int W, int dtype, void *stream)
{
    if (!x || !all_set(p) || !grad_y || !saved || !grad_x || !all_set(grads) || !workspace) return DLKA_ERR_NULL;
    DLKA_TRY(check_block(B, C, D, H, W));
    hipStream_t st = (hipStream_t)stream;
    return DLKA_DISPATCH(dtype,
                         lka3d_backward_t<float>(x, p, grad_y, saved, saved_bytes, grad_x, grads, workspace, workspace_bytes, B, C, D, H, W, dtype, st),
                         lka3d_backward_t<bf16_t>(x, p, grad_y, saved, saved_bytes, grad_x, grads, workspace, workspace_bytes, B, C, D, H, W, dtype, st));
}

// Which path a 2-D block call takes: the channels-last fast path wherever the width allows, unless the general NCHW kernels are forced.  ONE
// process-wide switch (initialised once from DLKA_LKA2D_GENERAL, changed only through dlka_lka2d_force_general), read by the size queries, the
// forward and the backward call alike — so a forward / backward pair and their buffer sizes cannot disagree because the environment changed in
// between.  Buffer sizes are the maximum over both paths: a switch between two calls never under-sizes a buffer.
static int g_lka2d_general = -1;
static bool lka2d_general()
{
    if (g_lka2d_general < 0) g_lka2d_general = getenv("DLKA_LKA2D_GENERAL") != nullptr ? 1 : 0;
    return g_lka2d_general != 0;
}
int dlka_lka2d_force_general(int on)
{
    const int old = lka2d_general() ? 1 : 0;
    g_lka2d_general = on ? 1 : 0;
    return old;
}

size_t dlka_lka2d_saved_bytes(int B, int C, int H, int W, int dtype)
{
    if (check_block(B, C, 1, H, W)) return 0;
    Lka2dGeoms G(B, C, H, W);
    size_t n = carved_bytes([&](Carver &m) { esz(dtype) == 2 ? (void)carve_lka2d_saved<bf16_t>(m, G) : (void)carve_lka2d_saved<float>(m, G); });
    if (lka2d_cl_supported(B, C, H, W, dtype)) n = std::max(n, lka2d_cl_saved_bytes(B, C, H, W, dtype));   // channels-last fast path (capi_lka2d_cl.hip)
    return n;
}

size_t dlka_lka2d_workspace_bytes(int B, int C, int H, int W, int dtype)
{
    if (check_block(B, C, 1, H, W)) return 0;
    Lka2dGeoms G(B, C, H, W);
    size_t n = esz(dtype) == 2 ? planar_workspace_bytes<bf16_t>(G, G.Off7, dtype) : planar_workspace_bytes<float>(G, G.Off7, dtype);
    if (lka2d_cl_supported(B, C, H, W, dtype)) n = std::max(n, lka2d_cl_workspace_bytes(B, C, H, W, dtype));
    return n;
}

int dlka_lka2d_attention_forward(const void *x, const dlka_lka2d_params *p, void *y, void *saved, size_t saved_bytes,
                                 void *workspace, size_t workspace_bytes, int B, int C, int H, int W, int dtype, void *stream)
{
    if (!x || !all_set(p) || !y || !saved || !workspace) return DLKA_ERR_NULL;
    DLKA_TRY(check_block(B, C, 1, H, W));
    hipStream_t st = (hipStream_t)stream;
    // channels-last fast path (MFMA offset nets, gather-layout depthwise deformable convs) wherever the width allows
    if (lka2d_cl_supported(B, C, H, W, dtype) && !lka2d_general())
        return lka2d_cl_forward(x, p, y, saved, saved_bytes, workspace, workspace_bytes, B, C, H, W, dtype, st);
    if (dtype == DLKA_BF16) return DLKA_ERR_UNSUPPORTED;   // DLKA_BF16 = bf16 activations with FP32 parameters: the channels-last path only
    return DLKA_DISPATCH(dtype, lka2d_forward_t<float>(x, p, y, saved, saved_bytes, workspace, workspace_bytes, B, C, H, W, st),
                         lka2d_forward_t<bf16_t>(x, p, y, saved, saved_bytes, workspace, workspace_bytes, B, C, H, W, st));
}

int dlka_lka2d_saved_offsets(int B, int C, int H, int W, int dtype, size_t byte_offsets[2], int *elem_bytes)
{
    if (!byte_offsets || !elem_bytes) return DLKA_ERR_NULL;
    DLKA_TRY(check_block(B, C, 1, H, W));
    if (lka2d_cl_supported(B, C, H, W, dtype) && !lka2d_general())
        return lka2d_cl_saved_offsets(B, C, H, W, dtype, byte_offsets, elem_bytes);
    if (dtype == DLKA_BF16) return DLKA_ERR_UNSUPPORTED;
    Carver sv = Carver::probing();
    const PlanarSaved2d<float> S = carve_lka2d_saved<float>(sv, Lka2dGeoms(B, C, H, W));   // (fp32 and, as fp32, float64: bf16 took the branch above)
    byte_offsets[0] = sv.offset_of(S.o5);
    byte_offsets[1] = sv.offset_of(S.o7);
    *elem_bytes = (int)esz(dtype);
    return DLKA_OK;
}

int dlka_lka2d_attention_backward(const void *x, const dlka_lka2d_params *p, const void *grad_y, const void *saved, size_t saved_bytes,
                                  void *grad_x, const dlka_lka2d_grads *grads, void *workspace, size_t workspace_bytes,
                                  int B, int C, int H, int W, int dtype, void *stream)
{
    if (!x || !all_set(p) || !grad_y || !saved || !grad_x || !all_set(grads) || !workspace) return DLKA_ERR_NULL;
    DLKA_TRY(check_block(B, C, 1, H, W));
    hipStream_t st = (hipStream_t)stream;
    if (lka2d_cl_supported(B, C, H, W, dtype) && !lka2d_general())
        return lka2d_cl_backward(x, p, grad_y, saved, saved_bytes, grad_x, grads, workspace, workspace_bytes, B, C, H, W, dtype, st);
    if (dtype == DLKA_BF16) return DLKA_ERR_UNSUPPORTED;
    return DLKA_DISPATCH(dtype,
                         lka2d_backward_t<float>(x, p, grad_y, saved, saved_bytes, grad_x, grads, workspace, workspace_bytes, B, C, H, W, dtype, st),
                         lka2d_backward_t<bf16_t>(x, p, grad_y, saved, saved_bytes, grad_x, grads, workspace, workspace_bytes, B, C, H, W, dtype, st));
}

}  // extern "C"
