// ---- TransformerBlock_3D_single_deform_LKA, one call per direction -----------------------------------------------------------
// Reference: 3D/d_lka_former/network_architecture/synapse/transformerblock.py:617-630 (forward), dynunet_block.py:66-80
// (UnetResBlock.forward).  Everything stays in token layout [M][C]; the only strided access is the read of an NCDHW input.
#include "capi_lka3d_tokens.h"

using namespace dlka;

extern "C" {

namespace {

struct TBlockGeoms {
    SameConv c3, pw;   // the 3^3 dense convs of UnetResBlock, the 1x1x1 conv of conv8
    size_t E, M;
    TokGeoms lka;      // the D-LKA attention inside
    mutable size_t lka_ws = 0;   // its workspace size (both workspace layouts start with it; measured on first use)
    size_t lka_ws_bytes() const { return lka_ws ? lka_ws : (lka_ws = tok_workspace_bytes(lka)); }
    TBlockGeoms(int B, int C, int D, int H, int W, int dtype, int variant) : lka(B, C, D, H, W, dtype, variant)
    {
        dlka_conv_geom g;
        memset(&g, 0, sizeof(g));
        g.B = B; g.C = C; g.D = D; g.H = H; g.W = W; g.Cout = C;
        g.kd = g.kh = g.kw = 3; g.sd = g.sh = g.sw = 1; g.pd = g.ph = g.pw = 1; g.dd = g.dh = g.dw = 1; g.group = 1; g.deformable_group = 1; g.im2col_step = 64;
        make_same_conv(&g, c3);
        g.kd = g.kh = g.kw = 1; g.pd = g.ph = g.pw = 0;
        make_same_conv(&g, pw);
        M = (size_t)c3.M;
        E = M * C;
    }
    size_t wp_floats() const { return dense_wp_floats(c3); }
    size_t part_floats() const { return cl_wgrad_part_floats(c3.M, c3.K, c3.Cout, c3.Cin); }
};

bool tblock_supported(int B, int C, int D, int H, int W, int variant = DLKA_LKA3D_SYNAPSE) { return tokens_supported(B, C, D, H, W, variant) && (long)D * H * W < (1l << 31); }

struct TBlockSaved {
    float *xt, *xn, *e, *attn, *c1, *a1, *c2, *rd, *lnstats;
    float *w1_f, *w1_b, *w2_f, *w2_b, *w8_f, *w8_b;   // prepared weights (forward / data-gradient forms), written by ONE launch in forward
    void *lka;
    size_t lka_bytes;
};

bool carve_tblock_saved(Carver &sv, const TBlockGeoms &G, TBlockSaved &S)
{
    S.xt = (float *)sv.take(G.E * 4); S.xn = (float *)sv.take(G.E * 4); S.e = (float *)sv.take(G.E * 4); S.attn = (float *)sv.take(G.E * 4);
    S.c1 = (float *)sv.take(G.E * 4); S.a1 = (float *)sv.take(G.E * 4); S.c2 = (float *)sv.take(G.E * 4); S.rd = (float *)sv.take(G.E * 4);
    S.lnstats = (float *)sv.take(G.M * 2 * 4);
    S.w1_f = (float *)sv.take(dense_wp_floats(G.c3) * 4); S.w1_b = (float *)sv.take(dense_wp_floats(G.c3) * 4);
    S.w2_f = (float *)sv.take(dense_wp_floats(G.c3) * 4); S.w2_b = (float *)sv.take(dense_wp_floats(G.c3) * 4);
    S.w8_f = (float *)sv.take(dense_wp_floats(G.pw) * 4); S.w8_b = (float *)sv.take(dense_wp_floats(G.pw) * 4);
    S.lka_bytes = tok_saved_bytes(G.lka);
    S.lka = sv.take(S.lka_bytes);   // TokSaved
    return sv.ok();
}

// `workspace`, both directions: the attention's own workspace in front, then what the wrapper's kernels use
struct TBlockFwdWs {
    void *lka;
    size_t lka_bytes;
    float *wp_reserve;   // (unused since the prepared weights moved into `saved`)
    float *sums;         // BatchNorm sums (atomics)
    float *xn32;         // mixed mode: LayerNorm's unrounded output, for the offset-determining chain of the attention.  Forward-only: it sits where the backward
                         // call's partial sums and gradient buffers will be
};
TBlockFwdWs carve_tblock_fwd_ws(Carver &cv, const TBlockGeoms &G, bool want_xn32)
{
    TBlockFwdWs W;
    W.lka_bytes = G.lka_ws_bytes();
    W.lka = cv.take(W.lka_bytes);
    W.wp_reserve = (float *)cv.take(G.wp_floats() * 4);
    W.sums = (float *)cv.take(4096);
    W.xn32 = want_xn32 ? (float *)cv.take(G.E * 4) : nullptr;
    return W;
}
struct TBlockBwdWs {
    void *lka, *lka_part;   // lka_part: the attention's partial sums when the pass is split (phase 1 / 2): outside its own workspace
    size_t lka_bytes, lka_part_bytes;
    float *wp_reserve, *part1, *part2, *part8;
    float *b[6];            // gradient buffers (the phased backward call says which gradient lives in which)
    float *sums;
};
TBlockBwdWs carve_tblock_bwd_ws(Carver &cv, const TBlockGeoms &G)
{
    TBlockBwdWs W;
    W.lka_bytes = G.lka_ws_bytes();
    W.lka = cv.take(W.lka_bytes);
    W.wp_reserve = (float *)cv.take(G.wp_floats() * 4);
    W.part1 = (float *)cv.take(G.part_floats() * 4); W.part2 = (float *)cv.take(G.part_floats() * 4);
    W.part8 = (float *)cv.take(cl_wgrad_part_floats(G.pw.M, 1, G.pw.Cout, G.pw.Cin) * 4);
    for (float *&b : W.b) b = (float *)cv.take(G.E * 4);
    W.sums = (float *)cv.take(4096);
    W.lka_part_bytes = G.lka.part_bytes;
    W.lka_part = cv.take(W.lka_part_bytes);
    return W;
}

}  // namespace

// dtype = DLKA_BF16 on the wrapper block is MIXED precision: x, y, the residual stream, LayerNorm / BatchNorm statistics, the 3^3 convs of UnetResBlock and
// every wrapper gradient stay fp32 (pointers are fp32 on both dtypes); the D-LKA attention inside (transformerblock.py:624) runs DLKA_BF16 — its input xn, output
// e and their gradients are bf16 storage, with the mixed-precision rule of the token path (fp32 offset-determining chain, fp32 parameters / accumulation).
int dlka_tblock3d_supported_v(int B, int C, int D, int H, int W, int dtype, int variant)
{
    return ((dtype == DLKA_F32 || dtype == DLKA_BF16) && tblock_supported(B, C, D, H, W, variant)) ? 1 : 0;
}
int dlka_tblock3d_supported(int B, int C, int D, int H, int W, int dtype) { return dlka_tblock3d_supported_v(B, C, D, H, W, dtype, DLKA_LKA3D_SYNAPSE); }

size_t dlka_tblock3d_saved_bytes(int B, int C, int D, int H, int W, int dtype) { return dlka_tblock3d_saved_bytes_v(B, C, D, H, W, dtype, DLKA_LKA3D_SYNAPSE); }
size_t dlka_tblock3d_saved_bytes_v(int B, int C, int D, int H, int W, int dtype, int variant)
{
    if (!dlka_tblock3d_supported_v(B, C, D, H, W, dtype, variant)) return 0;
    const TBlockGeoms G(B, C, D, H, W, dtype, variant);
    return carved_bytes([&](Carver &m) { TBlockSaved S; carve_tblock_saved(m, G, S); });
}

int dlka_tblock3d_saved_offsets_v(int B, int C, int D, int H, int W, int dtype, int variant, size_t *byte_offset)
{
    if (!byte_offset) return DLKA_ERR_NULL;
    if (!dlka_tblock3d_supported_v(B, C, D, H, W, dtype, variant)) return DLKA_ERR_UNSUPPORTED;
    const TBlockGeoms G(B, C, D, H, W, dtype, variant);
    Carver sv = Carver::probing();
    TBlockSaved S;
    carve_tblock_saved(sv, G, S);
    Carver lsv(S.lka, S.lka_bytes);
    *byte_offset = sv.offset_of(carve_tok_saved(lsv, G.lka).off);
    return DLKA_OK;
}

int dlka_tblock3d_saved_activations_v(int B, int C, int D, int H, int W, int dtype, int variant, size_t byte_offsets[2])
{
    if (!byte_offsets) return DLKA_ERR_NULL;
    if (!dlka_tblock3d_supported_v(B, C, D, H, W, dtype, variant)) return DLKA_ERR_UNSUPPORTED;
    Carver sv = Carver::probing();
    TBlockSaved S;
    carve_tblock_saved(sv, TBlockGeoms(B, C, D, H, W, dtype, variant), S);
    byte_offsets[0] = sv.offset_of(S.a1);
    byte_offsets[1] = sv.offset_of(S.rd);
    return DLKA_OK;
}

size_t dlka_tblock3d_workspace_bytes(int B, int C, int D, int H, int W, int dtype) { return dlka_tblock3d_workspace_bytes_v(B, C, D, H, W, dtype, DLKA_LKA3D_SYNAPSE); }
size_t dlka_tblock3d_workspace_bytes_v(int B, int C, int D, int H, int W, int dtype, int variant)
{
    if (!dlka_tblock3d_supported_v(B, C, D, H, W, dtype, variant)) return 0;
    const TBlockGeoms G(B, C, D, H, W, dtype, variant);
    const size_t f = carved_bytes([&](Carver &m) { carve_tblock_fwd_ws(m, G, true); });   // (xn32 at its capacity: the size does not depend on the mixed-mode switch)
    const size_t b = carved_bytes([&](Carver &m) { carve_tblock_bwd_ws(m, G); });
    return f > b ? f : b;
}

int dlka_tblock3d_forward(const void *x, int x_planar, const dlka_tblock3d_params *p, const dlka_lka3d_params *lka, const void *drop_mask, int training,
                          void *bn_stats, void *y, void *saved, size_t saved_bytes, void *workspace, size_t workspace_bytes, int B, int C, int D, int H, int W,
                          float ln_eps, float bn_eps, int dtype, void *stream)
{
    return dlka_tblock3d_forward_v(x, x_planar, p, lka, drop_mask, training, bn_stats, y, saved, saved_bytes, workspace, workspace_bytes, B, C, D, H, W, ln_eps, bn_eps,
                                   dtype, DLKA_LKA3D_SYNAPSE, stream);
}

int dlka_tblock3d_forward_v(const void *x, int x_planar, const dlka_tblock3d_params *p, const dlka_lka3d_params *lka, const void *drop_mask, int training,
                            void *bn_stats, void *y, void *saved, size_t saved_bytes, void *workspace, size_t workspace_bytes, int B, int C, int D, int H, int W,
                            float ln_eps, float bn_eps, int dtype, int variant, void *stream)
{
    if (!x || !p || !lka || !bn_stats || !y || !saved || !workspace) return DLKA_ERR_NULL;
    if (!p->norm_w || !p->norm_b || !p->gamma || !p->conv51_conv1_w || !p->conv51_conv2_w || !p->conv51_norm1_w || !p->conv51_norm1_b ||
        !p->conv51_norm2_w || !p->conv51_norm2_b || !p->conv8_w || !p->conv8_b)
        return DLKA_ERR_NULL;
    if (!dlka_tblock3d_supported_v(B, C, D, H, W, dtype, variant)) return DLKA_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const TBlockGeoms G(B, C, D, H, W, dtype, variant);
    Carver sv(saved, saved_bytes), cv(workspace, workspace_bytes);
    TBlockSaved S;
    if (!carve_tblock_saved(sv, G, S)) return DLKA_ERR_WORKSPACE;
    const int lo = dtype == DLKA_BF16 ? 1 : 0;   // the D-LKA attention runs DLKA_BF16: xn / e are bf16 storage
    static const bool xn32_on = [] { const char *e = getenv("DLKA_MIXED_XN32"); return !(e && e[0] == '0'); }();   // (A/B: 0 = the chain starts from the bf16 tensor, as in round 4)
    const TBlockFwdWs Wf = carve_tblock_fwd_ws(cv, G, lo && xn32_on);
    if (!cv.ok()) return DLKA_ERR_WORKSPACE;
    void *lka_ws = Wf.lka;
    const size_t lka_ws_bytes = Wf.lka_bytes;
    float *sums = Wf.sums, *xn32 = Wf.xn32;
    const long M = (long)G.M, N = G.c3.N;
    float *st1 = (float *)bn_stats, *st2 = st1 + 3 * C;
    const float slope = 0.01f;   // UnetResBlock's act_name default (dynunet_block.py:41)
    // ONE launch prepares the wrapper's six weight forms (kept in `saved` for the backward call) and zero-fills what this direction accumulates
    // into with atomics (BatchNorm sums, tap-split conv outputs)
    {
        PrepBatch pb;
        memset(&pb, 0, sizeof(pb));
        const int f3 = split_mode_flag(use_split(G.c3, true)), b3 = 1 | split_mode_flag(use_split(G.c3, false));
        add_job(pb, p->conv51_conv1_w, S.w1_f, C, C, 27, C, C, f3);
        add_job(pb, p->conv51_conv1_w, S.w1_b, C, C, 27, C, C, b3);
        add_job(pb, p->conv51_conv2_w, S.w2_f, C, C, 27, C, C, f3);
        add_job(pb, p->conv51_conv2_w, S.w2_b, C, C, 27, C, C, b3);
        add_job(pb, p->conv8_w, S.w8_f, C, C, 1, C, C, 0);
        add_job(pb, p->conv8_w, S.w8_b, C, C, 1, C, C, 1);
        auto add_zero = [&](float *ptr, size_t n) { PrepJob &j = pb.j[pb.njobs++]; memset(&j, 0, sizeof(j)); j.dst = ptr; j.n = (long)n; j.mode = 5; pb.total += j.n; };
        add_zero(sums, 1024);
        if (dense_forward_splits(G.c3, 0) > 1) { add_zero(S.c1, G.E); add_zero(S.c2, G.E); }
        if (dense_forward_splits(G.pw, 3) > 1) add_zero((float *)y, G.E);
        // ... and the attention's own fifteen forms go out with them (round 5: one launch per block less in the path the trainers call; the attention's zero fills ride
        // in its first kernel, as they do behind the engine's hoisted preparation)
        if (!all_set(lka)) return DLKA_ERR_NULL;
        Carver lsv(S.lka, S.lka_bytes);
        const TokSaved LS = carve_tok_saved(lsv, G.lka);
        if (!lsv.ok()) return DLKA_ERR_WORKSPACE;
        TokPrep PWl;
        DLKA_TRY(carve_prep(G.lka, LS.prep, PWl, lka, st, true, nullptr, &pb, true));
        DLKA_TRY(launch_cl_prep_batch(pb, st));
    }
    // tokens (+ pos_embed) and LayerNorm (:620-624)
    DLKA_TRY(launch_cl_layernorm_fwd((const float *)x, x_planar, (const float *)p->pos_embed, (const float *)p->norm_w, (const float *)p->norm_b, S.xt, S.xn,
                                     S.lnstats, B, (int)N, C, ln_eps, st, lo, xn32));
    // epa_block = the D-LKA block (:624)
    DLKA_TRY(tokens_forward_impl(S.xn, lka, S.e, S.lka, S.lka_bytes, lka_ws, lka_ws_bytes, B, C, D, H, W, dtype, stream, true, variant, xn32));   // (prepared above)
    // attn = x + gamma * epa (:624); attn IS attn_skip in channels-last memory (:626 is a view here)
    DLKA_TRY(launch_cl_scale_residual_fwd(S.xt, S.e, (const float *)p->gamma, S.attn, M, C, st, lo));
    // conv51 = UnetResBlock (dynunet_block.py:66-80)
    DLKA_TRY(dense_forward(G.c3, S.attn, nullptr, nullptr, S.c1, 0, S.w1_f, 0, nullptr, nullptr, st, true));
    // (batch statistics in their deterministic form: the attention's workspace is free again and serves as the per-workgroup partial-sum scratch)
    if (training) DLKA_TRY(launch_cl_bn_stats(S.c1, sums, st1, M, C, bn_eps, st, true, (float *)lka_ws, lka_ws_bytes / 4));
    DLKA_TRY(launch_cl_bn_apply(S.c1, nullptr, (const float *)p->conv51_norm1_w, (const float *)p->conv51_norm1_b, st1, nullptr, S.a1, M, N, C, slope, st));
    DLKA_TRY(dense_forward(G.c3, S.a1, nullptr, nullptr, S.c2, 0, S.w2_f, 0, nullptr, nullptr, st, true));
    if (training) DLKA_TRY(launch_cl_bn_stats(S.c2, sums + 512, st2, M, C, bn_eps, st, true, (float *)lka_ws, lka_ws_bytes / 4));
    // ... + residual, LeakyReLU, and conv8[0] = Dropout3d folded into the same pass (:611)
    DLKA_TRY(launch_cl_bn_apply(S.c2, S.attn, (const float *)p->conv51_norm2_w, (const float *)p->conv51_norm2_b, st2, (const float *)drop_mask, S.rd, M, N, C, slope, st));
    // x = attn_skip + conv8(attn) (:628)
    DLKA_TRY(dense_forward(G.pw, S.rd, nullptr, (const float *)p->conv8_b, (float *)y, 0, S.w8_f, 3, S.attn, nullptr, st, true));
    return DLKA_OK;
}

int dlka_tblock3d_backward(const dlka_tblock3d_params *p, const dlka_lka3d_params *lka, const void *drop_mask, int training, const void *bn_stats,
                           const void *grad_y, const void *saved, size_t saved_bytes, void *grad_x, const dlka_tblock3d_grads *gr,
                           const dlka_lka3d_grads *glka, void *workspace, size_t workspace_bytes, int B, int C, int D, int H, int W, int dtype, void *stream)
{
    return dlka_tblock3d_backward_v(p, lka, drop_mask, training, bn_stats, grad_y, saved, saved_bytes, grad_x, gr, glka, workspace, workspace_bytes, B, C, D, H, W, dtype,
                                    DLKA_LKA3D_SYNAPSE, stream);
}

int dlka_tblock3d_backward_v(const dlka_tblock3d_params *p, const dlka_lka3d_params *lka, const void *drop_mask, int training, const void *bn_stats,
                             const void *grad_y, const void *saved, size_t saved_bytes, void *grad_x, const dlka_tblock3d_grads *gr,
                             const dlka_lka3d_grads *glka, void *workspace, size_t workspace_bytes, int B, int C, int D, int H, int W, int dtype, int variant,
                             void *stream)
{
    return dlka_tblock3d_backward_phase_v(p, lka, drop_mask, training, bn_stats, grad_y, saved, saved_bytes, grad_x, gr, glka, workspace, workspace_bytes, B, C, D, H, W,
                                          dtype, variant, 0, stream);
}

// phase 0: the whole backward pass (dlka_tblock3d_backward_v).  phase 1: the DATA-gradient chain only — grad_x and every gradient a data kernel produces on its
// way (LayerNorm / BatchNorm affine parameters, gamma, pos_embed) — leaving in `workspace` what phase 2 reads; phase 2: the wrapper's three conv weight gradients, the
// attention's weight gradients and the fold of their partial sums, reading `workspace` as phase 1 left it.  A caller that issues phase 2 on another stream (behind an
// event recorded after phase 1, same `workspace`, which must stay untouched until phase 2 has run) lets a block's weight gradients overlap the NEXT block's data
// chain: what the block-stack engine does for the bare attention (dlka_lka3d_attention_tokens_backward_phase_v), here for the block the trainers call.
int dlka_tblock3d_backward_phase_v(const dlka_tblock3d_params *p, const dlka_lka3d_params *lka, const void *drop_mask, int training, const void *bn_stats,
                                   const void *grad_y, const void *saved, size_t saved_bytes, void *grad_x, const dlka_tblock3d_grads *gr,
                                   const dlka_lka3d_grads *glka, void *workspace, size_t workspace_bytes, int B, int C, int D, int H, int W, int dtype, int variant,
                                   int phase, void *stream)
{
    if (phase < 0 || phase > 2) return DLKA_ERR_SHAPE;
    if (!p || !lka || !bn_stats || !grad_y || !saved || !grad_x || !gr || !glka || !workspace) return DLKA_ERR_NULL;
    if (!gr->norm_w || !gr->norm_b || !gr->gamma || !gr->conv51_conv1_w || !gr->conv51_conv2_w || !gr->conv51_norm1_w || !gr->conv51_norm1_b ||
        !gr->conv51_norm2_w || !gr->conv51_norm2_b || !gr->conv8_w || !gr->conv8_b)
        return DLKA_ERR_NULL;
    if ((p->pos_embed != nullptr) != (gr->pos_embed != nullptr)) return DLKA_ERR_NULL;
    if (!dlka_tblock3d_supported_v(B, C, D, H, W, dtype, variant)) return DLKA_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const TBlockGeoms G(B, C, D, H, W, dtype, variant);
    Carver sv(saved, saved_bytes), cv(workspace, workspace_bytes);
    TBlockSaved S;
    if (!carve_tblock_saved(sv, G, S)) return DLKA_ERR_WORKSPACE;
    const TBlockBwdWs Wb = carve_tblock_bwd_ws(cv, G);
    if (!cv.ok()) return DLKA_ERR_WORKSPACE;
    void *lka_ws = Wb.lka, *lka_part = Wb.lka_part;
    const size_t lka_ws_bytes = Wb.lka_bytes, lka_part_bytes = Wb.lka_part_bytes;
    float *part1 = Wb.part1, *part2 = Wb.part2, *part8 = Wb.part8, *sums = Wb.sums;
    float *b0 = Wb.b[0], *b1 = Wb.b[1], *b2 = Wb.b[2], *b3 = Wb.b[3], *b4 = Wb.b[4], *b5 = Wb.b[5];
    const long M = (long)G.M, N = G.c3.N;
    const float *st1 = (const float *)bn_stats, *st2 = st1 + 3 * C;
    const float *gy = (const float *)grad_y, *mask = (const float *)drop_mask;
    const float slope = 0.01f;
    const int lo = dtype == DLKA_BF16 ? 1 : 0;   // g_e / g_xn are bf16 storage (the D-LKA attention ran DLKA_BF16)
    // (g_c1 lives in b0 — g_rd is dead by then —, not beside g_c2 in b1: phase 2 reads BOTH g_c2 and g_c1 after the data chain has finished)
    float *g_rd = b0, *g_c2 = b1, *g_skip = b2, *g_attn = b3, *g_a1 = b4, *g_c1 = b0, *g_e = b4, *g_xn = b5;
    if (phase == 2) {   // the weight gradients alone, from what phase 1 left in `workspace`
        FinalizeBatch fb2;
        memset(&fb2, 0, sizeof(fb2));
        DLKA_TRY(dense_backward_weight(G.pw, S.rd, gy, 0, (float *)gr->conv8_w, (float *)gr->conv8_b, part8, st, &fb2.j[fb2.njobs++]));
        DLKA_TRY(dense_backward_weight(G.c3, S.a1, g_c2, 0, (float *)gr->conv51_conv2_w, nullptr, part2, st, &fb2.j[fb2.njobs++]));
        DLKA_TRY(dense_backward_weight(G.c3, S.attn, g_c1, 0, (float *)gr->conv51_conv1_w, nullptr, part1, st, &fb2.j[fb2.njobs++]));
        FinalizeJob jobs[FIN_JOBS_PER_BLOCK];
        int nj = 0;
        DLKA_TRY(tokens_backward_impl(S.xn, lka, g_e, S.lka, S.lka_bytes, g_xn, glka, lka_ws, lka_ws_bytes, B, C, D, H, W, dtype, variant, stream, lka_part,
                                      lka_part_bytes, jobs, &nj, 2));
        if (fb2.njobs + nj > (int)(sizeof(fb2.j) / sizeof(fb2.j[0]))) return DLKA_ERR_UNSUPPORTED;
        for (int k = 0; k < nj; ++k) fb2.j[fb2.njobs++] = jobs[k];
        return launch_cl_wgrad_finalize(fb2, st);
    }
    // everything this direction accumulates into with atomics, zero-filled by ONE launch; the weight re-layouts were done by the forward call;
    // the three weight-gradient folds are ONE launch
    {
        ZeroBatch zb;
        memset(&zb, 0, sizeof(zb));
        zb.add(sums, 1024);
        zb.add((float *)gr->gamma, C);
        zb.add((float *)gr->norm_w, C);
        zb.add((float *)gr->norm_b, C);
        if (gr->pos_embed) zb.add((float *)gr->pos_embed, (size_t)N * C);
        if (dense_backward_data_splits(G.c3, 0) > 1) zb.add(g_a1, G.E);
        if (dense_backward_data_splits(G.c3, 3) > 1) zb.add(g_attn, G.E);
        DLKA_TRY(launch_zero_batch(zb, st));
    }
    FinalizeBatch fb;
    memset(&fb, 0, sizeof(fb));
    // conv8[1]:  y = W8 rd + b8 + attn
    if (phase == 0) DLKA_TRY(dense_backward_weight(G.pw, S.rd, gy, 0, (float *)gr->conv8_w, (float *)gr->conv8_b, part8, st, &fb.j[fb.njobs++]));
    DLKA_TRY(dense_backward_data(G.pw, gy, 0, nullptr, g_rd, S.w8_b, 0, nullptr, st, nullptr, nullptr, true));
    // Dropout3d + LeakyReLU + (BN2(c2) + attn):  g_c2, and everything that flows into attn so far:  g_skip = gy + g_pre
    DLKA_TRY(launch_cl_bn_bwd(g_rd, mask, S.c2, S.rd, (const float *)p->conv51_norm2_w, st2, sums, g_c2, g_skip, gy, (float *)gr->conv51_norm2_w,
                              (float *)gr->conv51_norm2_b, M, N, C, slope, training, st, true));
    // conv2
    if (phase == 0) DLKA_TRY(dense_backward_weight(G.c3, S.a1, g_c2, 0, (float *)gr->conv51_conv2_w, nullptr, part2, st, &fb.j[fb.njobs++]));
    DLKA_TRY(dense_backward_data(G.c3, g_c2, 0, nullptr, g_a1, S.w2_b, 0, nullptr, st, nullptr, nullptr, true));
    // LeakyReLU + BN1
    DLKA_TRY(launch_cl_bn_bwd(g_a1, nullptr, S.c1, S.a1, (const float *)p->conv51_norm1_w, st1, sums + 512, g_c1, nullptr, nullptr, (float *)gr->conv51_norm1_w,
                              (float *)gr->conv51_norm1_b, M, N, C, slope, training, st, true));
    // conv1:  g_attn = W1^T g_c1 + g_skip
    if (phase == 0) DLKA_TRY(dense_backward_weight(G.c3, S.attn, g_c1, 0, (float *)gr->conv51_conv1_w, nullptr, part1, st, &fb.j[fb.njobs++]));
    // (the fold of the three conv weight gradients above rides in the D-LKA block's finalize launch below: one dependent launch less per block)
    DLKA_TRY(dense_backward_data(G.c3, g_c1, 0, nullptr, g_attn, S.w1_b, 3, g_skip, st, nullptr, nullptr, true));
    // attn = xt + gamma * e
    DLKA_TRY(launch_cl_scale_residual_bwd(g_attn, S.e, (const float *)p->gamma, g_e, (float *)gr->gamma, M, C, st, true, lo));
    // epa_block
    if (phase == 1) {
        FinalizeJob jobs[FIN_JOBS_PER_BLOCK];
        int nj = 0;
        DLKA_TRY(tokens_backward_impl(S.xn, lka, g_e, S.lka, S.lka_bytes, g_xn, glka, lka_ws, lka_ws_bytes, B, C, D, H, W, dtype, variant, stream, lka_part, lka_part_bytes,
                                      jobs, &nj, 1));
    } else
        DLKA_TRY(tokens_backward_impl(S.xn, lka, g_e, S.lka, S.lka_bytes, g_xn, glka, lka_ws, lka_ws_bytes, B, C, D, H, W, dtype, variant, stream, nullptr, 0, nullptr,
                                      nullptr, 0, &fb));
    // LayerNorm (+ the residual branch g_attn), pos_embed
    DLKA_TRY(launch_cl_layernorm_bwd(g_xn, g_attn, S.xt, S.lnstats, (const float *)p->norm_w, (float *)grad_x, (float *)gr->norm_w, (float *)gr->norm_b,
                                     (float *)gr->pos_embed, B, (int)N, C, st, true, lo));
    return DLKA_OK;
}

}  // extern "C"
