// The token-layout 3-D D-LKA block's geometry and prepared-weight records, shared by the block's own entry points (capi_lka3d_tokens.hip) and the wrapper
// block that runs it inside (capi_tblock3d.hip).
#pragma once
#include "cl_host.h"

namespace dlka {

// ---- the token-layout 3-D block ----------------------------------------------------------------------------------------
inline SameConv block_conv(int B, int C, int Cout, int D, int H, int W, int k, int pad, int dil, int group, int act_bf16 = 0)
{
    SameConv s;
    s.act_bf16 = act_bf16;
    s.B = B; s.D = D; s.H = H; s.W = W; s.N = D * H * W; s.M = B * s.N; s.Cin = C; s.Cout = Cout; s.group = group;
    s.kd = s.kh = s.kw = k; s.pd = s.ph = s.pw = pad; s.dd = s.dh = s.dw = dil; s.K = k * k * k;
    return s;
}

// DLKA_BF16 is MIXED precision: bf16 storage for x, y, every saved activation and the intermediate gradients — except the chain that
// decides WHERE the deformable conv samples:  a = GELU(proj_1 x) -> t1 = DW5 a -> t = DW7 t1 -> offsets = Coff t  runs on fp32 tensors
// (a32, t1_32, t_32: forward-only workspace, never saved) with the fp32 path's own kernels, so that the predicted offsets equal the fp32
// block's to fp32 rounding.  floor() of a sampling coordinate is discontinuous: with bf16-stored a / t1 / t the offsets move by ~0.4 %, the
// samples within that distance of an integer coordinate change cell, and conv_offset / conv_spatial / conv0 / proj_1 gradients land
// 5e-2 .. 1.8e-1 from the fp32 block's (measured round 2; reproduced on the CPU by oracle.blocks with per-tensor storage flags:
// storing ONLY t in fp32 does not help — 1.1e-1 —, the whole chain does — 3e-3).  The dw convs also write the bf16 copies of t1 / t that the
// gathers and the backward pass read: the sampled VALUES and every gradient are smooth in those, 2^-9 rounding is inside the 2e-2 contract.
// The depthwise pair conv0 / conv_spatial of LKA3d_deform by net variant (include/dlka.h: dlka_lka3d_variant) and width:
//   SYNAPSE (synapse/transformerblock.py:637-638; also the pancreas copy): 5^3 pad 2, then 7^3 dilation 3 pad 9 at every width
//   ACDC (acdc/transformerblock.py:213-237): C <= 64: 5^3 pad 2, (5,7,7) dilation 3 pad (6,9,9); C = 128: 5^3 pad 2, (3,5,5) dilation (1,3,3)
//         pad (1,6,6); C = 256: 3^3 pad 1, 3^3 pad 1
// (kernel / pad / dilation triples are in the tensor's axis order: the reference's "H, W, D" = this file's D, H, W)
struct DwPairCfg { int k0[3], p0[3], d0[3], k1[3], p1[3], d1[3]; };
inline bool dw_pair_cfg(int variant, int C, DwPairCfg &c)
{
    auto set = [](int *dst, int a, int b, int cc) { dst[0] = a; dst[1] = b; dst[2] = cc; };
    if (variant == DLKA_LKA3D_SYNAPSE) {
        set(c.k0, 5, 5, 5); set(c.p0, 2, 2, 2); set(c.d0, 1, 1, 1); set(c.k1, 7, 7, 7); set(c.p1, 9, 9, 9); set(c.d1, 3, 3, 3);
        return true;
    }
    if (variant != DLKA_LKA3D_ACDC) return false;
    if (C == 32 || C == 64) { set(c.k0, 5, 5, 5); set(c.p0, 2, 2, 2); set(c.d0, 1, 1, 1); set(c.k1, 5, 7, 7); set(c.p1, 6, 9, 9); set(c.d1, 3, 3, 3); }
    else if (C == 128) { set(c.k0, 5, 5, 5); set(c.p0, 2, 2, 2); set(c.d0, 1, 1, 1); set(c.k1, 3, 5, 5); set(c.p1, 1, 6, 6); set(c.d1, 1, 3, 3); }
    else if (C == 256) { set(c.k0, 3, 3, 3); set(c.p0, 1, 1, 1); set(c.d0, 1, 1, 1); set(c.k1, 3, 3, 3); set(c.p1, 1, 1, 1); set(c.d1, 1, 1, 1); }
    else return false;
    return true;
}
inline SameConv dw_conv(int B, int C, int D, int H, int W, const int *k, const int *p, const int *d, int act_bf16)
{
    SameConv s;
    s.act_bf16 = act_bf16;
    s.B = B; s.D = D; s.H = H; s.W = W; s.N = D * H * W; s.M = B * s.N; s.Cin = C; s.Cout = C; s.group = C;
    s.kd = k[0]; s.kh = k[1]; s.kw = k[2]; s.pd = p[0]; s.ph = p[1]; s.pw = p[2]; s.dd = d[0]; s.dh = d[1]; s.dw = d[2]; s.K = k[0] * k[1] * k[2];
    return s;
}

// weight-gradient partial sums: in the backward workspace, or the caller's block-private area when the fold is deferred (dlka_lka3d_tokens_partials_bytes_v)
struct TokPartials { float *p2, *c1, *p1, *off, *dcn, *stage5, *stage7; };

struct TokGeoms {
    SameConv pw, dw5, dw7, offc, dcn;   // (dw5 / dw7: conv0 / conv_spatial, whatever their kernels are in the variant)
    SameConv dw5_f, dw7_f, offc_f, pw_f;   // the forward chain's geometries: == dw5 / dw7 / offc / pw on the fp32 path, their fp32-storage twins on DLKA_BF16
    size_t E, Off, GOff;   // GOff: the backward's internal grad_offset buffer, 96 channel planes per batch (packed layout, DeformBwdArgs::goff_cpad)
    size_t SB;             // bytes per activation element (4, or 2 on the DLKA_BF16 path)
    size_t part_bytes;     // size of the TokPartials layout (carve_partials, measured once here: both workspace layouts hold it)
    TokGeoms(int B, int C, int D, int H, int W, int dtype = DLKA_F32, int variant = DLKA_LKA3D_SYNAPSE)
    {
        const int bf = dtype == DLKA_BF16 ? 1 : 0;
        SB = bf ? 2 : 4;
        DwPairCfg dc;
        if (!dw_pair_cfg(variant, C, dc)) dw_pair_cfg(DLKA_LKA3D_SYNAPSE, C, dc);   // (callers check the variant with tokens_supported first)
        pw = block_conv(B, C, C, D, H, W, 1, 0, 1, 1, bf);
        dw5 = dw_conv(B, C, D, H, W, dc.k0, dc.p0, dc.d0, bf);
        dw7 = dw_conv(B, C, D, H, W, dc.k1, dc.p1, dc.d1, bf);
        offc = block_conv(B, C, 81, D, H, W, 3, 1, 1, 1, bf);
        dcn = block_conv(B, C, C, D, H, W, 3, 1, 1, 1, bf);
        dw5_f = dw_conv(B, C, D, H, W, dc.k0, dc.p0, dc.d0, 0);
        dw7_f = dw_conv(B, C, D, H, W, dc.k1, dc.p1, dc.d1, 0);
        offc_f = block_conv(B, C, 81, D, H, W, 3, 1, 1, 1, 0);
        pw_f = block_conv(B, C, C, D, H, W, 1, 0, 1, 1, 0);
        E = (size_t)B * C * D * H * W;
        Off = (size_t)B * 81 * D * H * W;
        GOff = (size_t)B * 96 * D * H * W;
        part_bytes = carved_bytes([&](Carver &m) { carve_partials(m); });
    }
    size_t wp_floats() const
    {
        size_t m = dense_wp_floats(offc);
        if (dense_wp_floats(dcn) > m) m = dense_wp_floats(dcn);
        if ((size_t)dw7.K * dw7.Cin > m) m = (size_t)dw7.K * dw7.Cin;
        return m;
    }
    size_t scratch_floats() const { return deform_scratch_floats(dcn); }
    // class-blocked fp32 copy of a depthwise conv's input (cl_dwconv_lds.hip): two of them, so that one conv's epilogue can write the next one's
    size_t blk_floats() const
    {
        const size_t a5 = cl_dwconv_blk_floats(dw5.B, dw5.Cin, dw5.D, dw5.H, dw5.W, dw5.dw), a7 = cl_dwconv_blk_floats(dw7.B, dw7.Cin, dw7.D, dw7.H, dw7.W, dw7.dw);
        return ((a5 > a7 ? a5 : a7) + 63) & ~(size_t)63;
    }
    // the deformable conv's samples S[tap][m][c], handed from the grad_offset kernel to the weight gradient (0: too large for 32-bit buffer
    // offsets, or switched off — the weight gradient then gathers for itself).  The switch is ONE process-wide value (wgrad_gather(): initialised once
    // from DLKA_WGRAD_GATHER, changed only through dlka_lka3d_force_wgrad_gather), and the workspace SIZE query always includes the sample area
    // (samp_capacity_floats), so flipping the switch between sizing and a backward call can never under-size a buffer (round-3 verdict).
    size_t samp_capacity_floats() const
    {
        const size_t n = (size_t)dcn.K * dcn.M * dcn.Cin;   // elements of the activation storage type (SB bytes each)
        return (n * SB < ((size_t)1 << 31)) ? n * SB / 4 : 0;
    }
    // prepared weights, kept in `saved` from the forward to the backward call (floats)
    size_t pw_floats() const { return (size_t)pw.Cin * pw.Cin; }
    size_t offc_floats() const { return dense_wp_floats(offc); }
    size_t dcn_floats() const { return dense_wp_floats(dcn); }
    size_t dw5_floats() const { return (size_t)dw5.K * dw5.Cin; }
    size_t dw7_floats() const { return (size_t)dw7.K * dw7.Cin; }
    size_t prep_floats() const { return 6 * pw_floats() + 2 * offc_floats() + 3 * dcn_floats() + 2 * dw5_floats() + 2 * dw7_floats() + 17 * 64; }
    // weight-gradient partials: every gradient of the block has its own area (folded by one fused launch at the end)
    size_t part_pw() const { return (cl_wgrad_part_floats_mode(pw.M, 1, pw.Cin, pw.Cin, 0) + 63) & ~(size_t)63; }
    size_t part_off() const { return (cl_wgrad_part_floats_mode(pw.M, 27, 81, pw.Cin, 0) + 63) & ~(size_t)63; }
    size_t part_dcn() const { return (cl_wgrad_part_floats_mode(pw.M, 27, pw.Cin, pw.Cin, 1) + 63) & ~(size_t)63; }
    size_t stage_dw() const { return (size_t)(dw5.K + 1 + dw7.K + 1) * pw.Cin; }   // conv0 [K0 + 1][C] then conv_spatial [K1 + 1][C]
    TokPartials carve_partials(Carver &pc) const
    {
        TokPartials P;
        P.p2 = (float *)pc.take(part_pw() * 4); P.c1 = (float *)pc.take(part_pw() * 4); P.p1 = (float *)pc.take(part_pw() * 4);
        P.off = (float *)pc.take(part_off() * 4);
        P.dcn = (float *)pc.take(part_dcn() * 4);
        P.stage5 = (float *)pc.take(stage_dw() * 4);   // the depthwise staging is ONE area (one zero fill): conv_spatial's rows follow conv0's
        P.stage7 = P.stage5 ? P.stage5 + (size_t)(dw5.K + 1) * pw.Cin : nullptr;
        return P;
    }
};

// carve + (forward only) fill the prepared-weight area
struct TokPrep {
    float *pw_f[3], *pw_b[3];   // proj_1, conv1, proj_2: forward (mode 0) / data-gradient (mode 1) layouts
    float *off_f, *off_b, *dcn_f, *dcn_b, *dw5_f, *dw5_b, *dw7_f, *dw7_b;
    float *dcn_b16;   // bf16 path: the deformable conv's column-matrix weights as two-term bf16 records (grad_offset / grad_input on the bf16 matrix cores)
};

// ---- the block's buffer layouts: one record and ONE carve function per buffer and direction (Carver, cl_host.h) ---------------------------------
// `saved`, forward to backward call.  Activation-typed (bf16 on DLKA_BF16) except the fp32 offsets and prepared weights.  Sized without slack.
struct TokSaved {
    float *h, *a, *t1, *t, *off, *f, *g1;
    float *prep;   // the prepared weights (carve_prep)
    float *m;      // gate output, kept: proj_2's weight gradient needs it
};
inline TokSaved carve_tok_saved(Carver &sv, const TokGeoms &G)
{
    const size_t act = G.E * G.SB;
    TokSaved S;
    S.h = (float *)sv.take(act); S.a = (float *)sv.take(act); S.t1 = (float *)sv.take(act); S.t = (float *)sv.take(act);
    S.off = (float *)sv.take(G.Off * 4);
    S.f = (float *)sv.take(act); S.g1 = (float *)sv.take(act);
    S.prep = (float *)sv.take(G.prep_floats() * 4);
    S.m = (float *)sv.take(act);
    return S;
}
inline size_t tok_saved_bytes(const TokGeoms &G) { return carved_bytes([&](Carver &m) { carve_tok_saved(m, G); }); }

// blocked inputs of the opt-in LDS-brick depthwise convs (DLKA_DW_LDS), both directions: sized and carved only when that mode is on — and only when both fit,
// so a mode switched on between the size query and the call keeps the register-row kernels instead of overrunning the workspace
inline void carve_tok_blk(Carver &cv, const TokGeoms &G, float *&blkA, float *&blkB)
{
    const bool want_blk = cl_dwconv_lds_mode() != 0;
    blkA = (float *)cv.take_opt(G.blk_floats() * 4, want_blk);
    blkB = (float *)cv.take_opt(G.blk_floats() * 4, want_blk && cv.got(blkA));
    if (!blkB) blkA = nullptr;
}

// `workspace`, backward call (the front of the buffer; the tail is TokWsTail)
struct TokBwdWs {
    float *wp_reserve;   // (unused since the prepared weights moved into `saved`; the sizes it contributes to are kept)
    float *part;         // TokPartials, unless the caller brings a block-private area
    // every intermediate gradient has its own buffer: the weight-gradient stream reads them while the data-gradient chain moves on.  fp32-sized on both
    // dtypes: gta and the split scratch ARE fp32
    float *gg1, *ga1, *gf, *gta, *gt, *gt1, *ga2, *gh;
    float *goff, *scratch;
    float *samp;         // ALWAYS carved at its capacity: the layout behind it does not depend on the gather switch (halves use its first half and one word behind: samp_f16_maxbits)
    float *blkA, *blkB;
    float *padt;         // the zero-padded copy of t the offset conv's weight gradient reads (null when the workspace was sized without it: the unpadded kernels)
};
inline TokBwdWs carve_tok_bwd_ws(Carver &cv, const TokGeoms &G)
{
    TokBwdWs W;
    W.wp_reserve = (float *)cv.take(G.wp_floats() * 4);
    W.part = (float *)cv.take(G.part_bytes);
    float **grad[8] = {&W.gg1, &W.ga1, &W.gf, &W.gta, &W.gt, &W.gt1, &W.ga2, &W.gh};
    for (float **g : grad) *g = (float *)cv.take(G.E * 4);
    W.goff = (float *)cv.take(G.GOff * 4);
    W.scratch = (float *)cv.take(G.scratch_floats() * 4);
    W.samp = G.samp_capacity_floats() ? (float *)cv.take(G.samp_capacity_floats() * 4) : nullptr;
    carve_tok_blk(cv, G, W.blkA, W.blkB);
    const size_t pad = dense_wgrad_pad_bytes(G.offc);
    W.padt = (float *)cv.take_opt(pad, pad != 0);
    return W;
}

// `workspace`, forward call (front).  Forward-only tensors, dead when the call returns; they sit where the backward call's gradient buffers gg1 .. gt will be,
// so that the forward pass never needs more than the backward pass does.
struct TokFwdWs {
    float *wp_reserve, *part_reserve, *gg1_reserve;   // (nothing of the forward pass lives here)
    float *a32, *t1_32, *t_32;                        // bf16 path: the fp32 offset-determining chain (TokGeoms)
    float *blkA, *blkB;
};
inline TokFwdWs carve_tok_fwd_ws(Carver &cv, const TokGeoms &G)
{
    TokFwdWs W;
    W.wp_reserve = (float *)cv.take(G.wp_floats() * 4);
    W.part_reserve = (float *)cv.take(G.part_bytes);
    W.gg1_reserve = (float *)cv.take(G.E * 4);
    W.a32 = (float *)cv.take(G.E * 4); W.t1_32 = (float *)cv.take(G.E * 4); W.t_32 = (float *)cv.take(G.E * 4);
    carve_tok_blk(cv, G, W.blkA, W.blkB);
    return W;
}

// `workspace`, the tail: behind everything either direction carves from the front.  Continues a forward carve (cv stands at the forward call's end)
struct TokWsTail {
    void *reserve;   // 4096 bytes nothing uses (the size queries have always counted them; memory use is behaviour)
    float *slab;     // forward pass, small stages: the deformable conv's tap-range slabs (null: none needed)
};
inline TokWsTail carve_tok_ws_tail(Carver &cv, const TokGeoms &G)
{
    cv.skip_to(carved_bytes([&](Carver &m) { carve_tok_bwd_ws(m, G); }));
    TokWsTail T;
    T.reserve = cv.take(4096);
    T.slab = deform_fwd_slab_floats(G.dcn) ? (float *)cv.take(deform_fwd_slab_floats(G.dcn) * 4) : nullptr;
    return T;
}
inline size_t tok_workspace_bytes(const TokGeoms &G)
{
    return carved_bytes([&](Carver &m) { carve_tok_fwd_ws(m, G); carve_tok_ws_tail(m, G); });
}

// (capi_lka3d_tokens.hip)
bool tokens_supported(int B, int C, int D, int H, int W, int variant = DLKA_LKA3D_SYNAPSE);
// collect != null: the jobs go into *collect instead of a launch — replacing its contents, or (append) behind the jobs it already holds
int carve_prep(const TokGeoms &G, float *base, TokPrep &t, const dlka_lka3d_params *p, hipStream_t st, bool fill, const ZeroBatch *zb = nullptr,
               PrepBatch *collect = nullptr, bool append = false);
constexpr int FIN_JOBS_PER_BLOCK = 8;   // weight-gradient folds one block hands to the finalisation
int tokens_forward_impl(const void *x_, const dlka_lka3d_params *p, void *y_, void *saved, size_t saved_bytes, void *workspace,
                        size_t workspace_bytes, int B, int C, int D, int H, int W, int dtype, void *stream, bool prepared,
                        int variant = DLKA_LKA3D_SYNAPSE, const float *x_f32 = nullptr);
int tokens_backward_impl(const void *x_, const dlka_lka3d_params *p, const void *gy_, const void *saved, size_t saved_bytes, void *gx_,
                         const dlka_lka3d_grads *gr, void *workspace, size_t workspace_bytes, int B, int C, int D, int H, int W, int dtype, int variant,
                         void *stream, void *partials, size_t partials_bytes, FinalizeJob *jobs_out, int *njobs_out, int phase = 0,
                         const FinalizeBatch *extra = nullptr);
}  // namespace dlka
