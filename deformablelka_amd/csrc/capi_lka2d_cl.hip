// =========================================================================================================================
// The 2-D D-LKA block (deformable_LKA_Attention, 2D/deformable_LKA/deformable_LKA.py:124-140) on the channels-last kernels.
// x / y arrive in the reference's NCHW layout; the block transposes once on the way in and once on the way out (two passes of E
// floats against ~100 E of work) and runs entirely in [B][H][W][C]:
//   1x1 projections (+GELU / gate / residual epilogues)      cl_pointwise_kernel: the frame shared with the plain block, capi_lka2d_frame.h — the frame is changed THERE; here only the spatial stage and the buffers
//   offset nets C -> 50 (5x5) and C -> 98 (7x7 dil 3)        cl_igemm_kernel (3-D kernel with D = kd = 1), planar offsets as torchvision wants them;
//                                                            split-bf16 MFMA as in the 3-D block (forward fp32-equivalent three-term)
//   the two depthwise deformable convs                       cl_ddw2d.hip
// Supported: fp32, C / 32 in {1, 2, 3, 4, 6, 8, 12} (the net's 96 / 192 / 384 / 768 -> the first three; 768 never runs).
// =========================================================================================================================
#include "capi_lka2d_frame.h"
#include "cl_fork.h"

using namespace dlka;

namespace dlka {

namespace {

// DLKA_BF16 (BASELINE.json config 2: "224x224 bf16 training, batch 24") is MIXED precision, like the 3-D block (TokGeoms): bf16 storage for x, y,
// every saved activation and the intermediate gradients — except the chain that decides WHERE the two deformable convs sample:
//     a = GELU(proj_1 x)  ->  o5 = offnet5(a)  ->  t1 = DDW5(a, o5)  ->  o7 = offnet7(t1)
// runs on fp32 tensors (a32, t1_32: forward-only workspace) with the fp32 path's own kernels, so that both offset fields equal the fp32 block's to
// fp32 rounding.  The bf16 copies of a / t1 (saved for the backward pass) ride in the producing kernels.
struct Lka2dCl : Lka2dFrame {
    SameConv off5, off7;          // activation-typed (bf16 on DLKA_BF16): the offset nets' backward passes
    SameConv off5_f, off7_f;      // the offset nets' FORWARD passes: fp32 input on both paths
    size_t O5, O7;
    Lka2dCl(int B_, int C_, int H_, int W_, int dtype) : Lka2dFrame(B_, C_, H_, W_, dtype)
    {
        off5 = block_conv2d(B, C, 50, H, W, 5, 2, 1, bf);
        off7 = block_conv2d(B, C, 98, H, W, 7, 9, 3, bf);
        off5_f = block_conv2d(B, C, 50, H, W, 5, 2, 1, 0);
        off7_f = block_conv2d(B, C, 98, H, W, 7, 9, 3, 0);
        O5 = (size_t)B * 50 * H * W; O7 = (size_t)B * 98 * H * W;
    }
    size_t off5_floats() const { return dense_wp_floats(off5); }
    size_t off7_floats() const { return dense_wp_floats(off7); }
    size_t prep_floats() const { return 6 * (pw_floats() + 64) + 2 * (off5_floats() + 64) + 2 * (off7_floats() + 64) + (size_t)(25 + 49) * C + 256; }
    size_t part_o5() const { return (cl_wgrad_part_floats_mode(pw.M, 25, 50, C, 0) + 63) & ~(size_t)63; }
    size_t part_o7() const { return (cl_wgrad_part_floats_mode(pw.M, 49, 98, C, 0) + 63) & ~(size_t)63; }
    size_t part_dw() const { return (cl_ddw2d_part_floats(pw.M, 49, C) + 63) & ~(size_t)63; }
    size_t part_floats() const { return 3 * part_pw() + part_o5() + part_o7() + part_dw(); }
};

struct Prep2d : FramePrep { float *o5_f, *o5_b, *o7_f, *o7_b, *dw5, *dw7; };

int carve_prep2d(const Lka2dCl &G, float *base, Prep2d &t, const dlka_lka2d_params *p, hipStream_t st, bool fill)
{
    PrepTake take{base};
    PrepBatch pb;
    memset(&pb, 0, sizeof(pb));
    const int C = G.C;
    carve_frame_prep(G, take, t, p, pb);
    t.o5_f = take(G.off5_floats()); t.o5_b = take(G.off5_floats());
    t.o7_f = take(G.off7_floats()); t.o7_b = take(G.off7_floats());
    t.dw5 = take((size_t)25 * G.C); t.dw7 = take((size_t)49 * G.C);
    if (!fill) return DLKA_OK;
    add_job(pb, p->conv0_offset_w, t.o5_f, 50, C, 25, C, 64, split_mode_flag(use_split(G.off5_f, true)));
    add_job(pb, p->conv0_offset_w, t.o5_b, 50, C, 25, 64, C, use_split(G.off5, false) ? 9 : 1);
    add_job(pb, p->conv_spatial_offset_w, t.o7_f, 98, C, 49, C, 128, split_mode_flag(use_split(G.off7_f, true)));
    add_job(pb, p->conv_spatial_offset_w, t.o7_b, 98, C, 49, 128, C, use_split(G.off7, false) ? 9 : 1);
    add_job(pb, p->conv0_w, t.dw5, C, C, 25, 0, 0, 3);
    add_job(pb, p->conv_spatial_w, t.dw7, C, C, 49, 0, 0, 3);
    return launch_cl_prep_batch(pb, st);
}

// ---- the block's buffer layouts: one record and ONE carve function per buffer and direction (Carver, cl_host.h) ---------------------------------
// `saved`: the frame's activation-typed tensors and one more nothing uses, the two offset fields (fp32 on both paths), the prepared weights
struct Lka2dSaved : FrameSaved { float *spare, *o5, *o7, *prep; };
Lka2dSaved carve_lka2d_saved(Carver &sv, const Lka2dCl &G)
{
    Lka2dSaved S;
    S.carve(sv, G);
    S.spare = (float *)sv.take(G.E * G.SB);
    S.o5 = (float *)sv.take(G.O5 * 4); S.o7 = (float *)sv.take(G.O7 * 4);
    S.prep = (float *)sv.take(G.prep_floats() * 4);
    return S;
}
// `workspace`, forward call: forward-only tensors where the backward call's first gradient buffers will be
struct Lka2dFwdWs { float *yt, *a32, *t1_32; };   // a32, t1_32: bf16 path, the fp32 offset-determining chain
Lka2dFwdWs carve_lka2d_fwd_ws(Carver &cv, const Lka2dCl &G)
{
    Lka2dFwdWs W;
    W.yt = (float *)cv.take(G.E * 4); W.a32 = (float *)cv.take(G.E * 4); W.t1_32 = (float *)cv.take(G.E * 4);
    return W;
}
// `workspace`, backward call.  The nine gradient buffers keep their fp32 size on the bf16 path: the two grad_input accumulators ARE fp32, others serve as
// landing zones of tap-split sums.
struct Lka2dBwdWs {
    float *gyt, *gg1, *ga1, *gt2, *gta, *gt1, *gaa, *gab, *gh;
    float *goff;     // the 7x7 conv's grad_offset
    float *goff5;    // the 5x5 conv's, in a buffer of its own: the 7x7 offset net's weight gradient may still be reading `goff`
    float *part;
    void *reserve;   // 4096 bytes nothing uses (the size query has always counted them)
    float *pad7, *pad5;   // the zero-padded copies the offset nets' weight gradients read (own buffers: both may be in flight on the internal stream at once)
};
Lka2dBwdWs carve_lka2d_bwd_ws(Carver &cv, const Lka2dCl &G)
{
    Lka2dBwdWs W;
    float **grad[9] = {&W.gyt, &W.gg1, &W.ga1, &W.gt2, &W.gta, &W.gt1, &W.gaa, &W.gab, &W.gh};
    for (float **g : grad) *g = (float *)cv.take(G.E * 4);
    W.goff = (float *)cv.take(G.O7 * 4);
    W.goff5 = (float *)cv.take(G.O5 * 4);
    W.part = (float *)cv.take(G.part_floats() * 4);
    W.reserve = cv.take(4096);
    W.pad7 = (float *)cv.take_opt(dense_wgrad_pad_bytes(G.off7), dense_wgrad_pad_bytes(G.off7) != 0);
    W.pad5 = (float *)cv.take_opt(dense_wgrad_pad_bytes(G.off5), dense_wgrad_pad_bytes(G.off5) != 0);
    return W;
}

void fill_ddw(DwArgs2d &d, const Lka2dCl &G, int k, int pad, int dil)
{
    memset(&d, 0, sizeof(d));
    d.B = G.B; d.H = G.H; d.W = G.W; d.C = G.C; d.kh = d.kw = k; d.ph = d.pw = pad; d.dh = d.dw = dil;
}

}  // namespace

int lka2d_cl_supported(int B, int C, int H, int W, int dtype)
{
    if ((dtype != DLKA_F32 && dtype != DLKA_BF16) || B <= 0 || H <= 0 || W <= 0 || !frame_width_ok(C) || !cl_ddw2d_supported(C)) return 0;
    if (!(nt_ok(C) || C == 192 || C == 384)) return 0;   // the offset nets' data gradient has C columns: the igemm launcher's tile menu
    if ((long)B * H * W * C >= (1l << 29)) return 0;
    return dense_fwd_supported(block_conv2d(B, C, 50, H, W, 5, 2, 1)) ? 1 : 0;
}

size_t lka2d_cl_saved_bytes(int B, int C, int H, int W, int dtype)
{
    const Lka2dCl G(B, C, H, W, dtype);
    return carved_bytes([&](Carver &m) { carve_lka2d_saved(m, G); });
}

// (diagnostics) the offset tensors inside `saved`
int lka2d_cl_saved_offsets(int B, int C, int H, int W, int dtype, size_t byte_offsets[2], int *elem_bytes)
{
    Carver sv = Carver::probing();
    const Lka2dSaved S = carve_lka2d_saved(sv, Lka2dCl(B, C, H, W, dtype));
    byte_offsets[0] = sv.offset_of(S.o5);
    byte_offsets[1] = sv.offset_of(S.o7);
    *elem_bytes = 4;
    return DLKA_OK;
}

size_t lka2d_cl_workspace_bytes(int B, int C, int H, int W, int dtype)
{
    const Lka2dCl G(B, C, H, W, dtype);
    const size_t f = carved_bytes([&](Carver &m) { carve_lka2d_fwd_ws(m, G); }), b = carved_bytes([&](Carver &m) { carve_lka2d_bwd_ws(m, G); });
    return f > b ? f : b;
}

int lka2d_cl_forward(const void *x_, const dlka_lka2d_params *p, void *y_, void *saved, size_t saved_bytes, void *workspace, size_t workspace_bytes, int B,
                     int C, int H, int W, int dtype, hipStream_t st)
{
    Lka2dCl G(B, C, H, W, dtype);
    const int bf = G.bf;
    Carver sv(saved, saved_bytes), cv(workspace, workspace_bytes);
    const Lka2dSaved S = carve_lka2d_saved(sv, G);
    const Lka2dFwdWs Wf = carve_lka2d_fwd_ws(cv, G);
    if (!sv.ok() || !cv.ok()) return DLKA_ERR_WORKSPACE;
    float *a = S.a, *t1 = S.t1, *t2 = S.t2, *o5 = S.o5, *o7 = S.o7, *prep = S.prep;
    float *a32 = Wf.a32, *t1_32 = Wf.t1_32;
    const float *N0 = nullptr;
    Prep2d PW;
    DLKA_TRY(carve_prep2d(G, prep, PW, p, st, true));
    DLKA_TRY(frame_forward_head(G, PW, x_, p->proj_1_b, S, bf ? a32 : nullptr, st));                                           // :135-136 proj_1 (+GELU)
    const float *a_in = bf ? a32 : a;
    DLKA_TRY(dense_forward(G.off5_f, a_in, N0, (const float *)p->conv0_offset_b, o5, 1, PW.o5_f, 0, nullptr, nullptr, st));     // :28 offset_net
    DwArgs2d d;
    fill_ddw(d, G, 5, 2, 1);
    d.in = a_in; d.off = o5; d.wp = PW.dw5; d.out = bf ? t1_32 : t1; d.out_lo = bf ? t1 : nullptr;
    DLKA_TRY(launch_cl_ddw2d_fwd(d, st));                                                                                     // :29
    const float *t1_in = bf ? t1_32 : t1;
    DLKA_TRY(dense_forward(G.off7_f, t1_in, N0, (const float *)p->conv_spatial_offset_b, o7, 1, PW.o7_f, 0, nullptr, nullptr, st));
    fill_ddw(d, G, 7, 9, 3);
    d.in = t1_in; d.off = o7; d.wp = PW.dw7; d.out = bf ? nullptr : t2; d.out_lo = bf ? t2 : nullptr;
    DLKA_TRY(launch_cl_ddw2d_fwd(d, st));
    return frame_forward_tail(G, PW, p->conv1_b, p->proj_2_b, S, Wf.yt, y_, st);                                           // :102-104 conv1 + gate, :138-139 proj_2 + shortcut
}

int lka2d_cl_backward(const void *x_, const dlka_lka2d_params *p, const void *gy_, const void *saved, size_t saved_bytes, void *gx_, const dlka_lka2d_grads *gr,
                      void *workspace, size_t workspace_bytes, int B, int C, int H, int W, int dtype, hipStream_t st)
{
    (void)x_;
    Lka2dCl G(B, C, H, W, dtype);
    const int bf = G.bf;
    Carver sv(saved, saved_bytes), cv(workspace, workspace_bytes);
    const Lka2dSaved S = carve_lka2d_saved(sv, G);
    const Lka2dBwdWs Wb = carve_lka2d_bwd_ws(cv, G);
    if (!sv.ok() || !cv.ok()) return DLKA_ERR_WORKSPACE;
    const float *a = S.a, *t1 = S.t1, *o5 = S.o5, *o7 = S.o7;
    float *gyt = Wb.gyt, *gg1 = Wb.gg1, *ga1 = Wb.ga1, *gt2 = Wb.gt2, *gta = Wb.gta, *gt1 = Wb.gt1, *gaa = Wb.gaa, *gab = Wb.gab, *gh = Wb.gh;
    float *goff = Wb.goff, *goff5 = Wb.goff5, *part = Wb.part, *pad7 = Wb.pad7, *pad5 = Wb.pad5;
    const float *N0 = nullptr;
    Prep2d PW;
    DLKA_TRY(carve_prep2d(G, S.prep, PW, p, st, false));
    // The two offset nets' WEIGHT gradients (the largest kernels of this pass after grad_input: C -> 98 / 50 channels over 49 / 25 taps) only read grad_offset and a saved
    // activation, and nothing before the finalisation reads their partial sums: they run on the library's internal stream (aux_ctx) beside the data chain — fork behind
    // each depthwise deformable conv's backward, one join in front of the finalisation.  DLKA_LKA2D_FORK=0: one stream (A/B; read per call).  Measured in
    // profiles/r06_notes.md.
    int fork_mode = 0;
#if !defined(HIPEMU)
    fork_mode = fork_env().lka2d_fork;
#endif
    ForkLease lease(st, fork_mode != 0);   // (joins whatever is still forked when a DLKA_TRY below returns early)
    const bool fork2d = lease.ok();
    // ... and each depthwise deformable conv's grad_input (the pass's largest kernel) beside its grad_offset / weight-gradient kernel on a second internal stream:
    // fork in front of the pair, join in front of the offset net's data gradient, which adds grad_input (DLKA_LKA2D_FORK=1: the weight gradients only)
    const bool forkgx = fork2d && fork_mode == 2;
    hipStream_t gst = forkgx ? lease.stream(2) : nullptr;
    auto fork_gx = [&]() -> int { return forkgx ? lease.fork(2) : DLKA_OK; };
    auto join_gx = [&]() -> int { return forkgx ? lease.join(2) : DLKA_OK; };
    hipStream_t wst = fork2d ? lease.stream(1) : st;
    auto fork_to_aux = [&]() -> int { return fork2d ? lease.fork(1) : DLKA_OK; };
    float *const part_pw[3] = {part, part + G.part_pw(), part + 2 * G.part_pw()};   // proj_2, conv1, proj_1
    float *part_o5 = part + 3 * G.part_pw(), *part_o7 = part_o5 + G.part_o5(), *part_dw = part_o7 + G.part_o7();
    FinalizeBatch fb;
    memset(&fb, 0, sizeof(fb));
    // bf16: the fp32 landing zone of a tap-split offset-net data gradient (converted into its bf16 destination afterwards): gg1 is dead by then for
    // the first one, gt2 for the second
    ZeroBatch zb;
    memset(&zb, 0, sizeof(zb));
    zb.add(gta, G.E);   // grad_input targets of the two depthwise deformable convs (fp32 atomics)
    zb.add(gaa, G.E);
    const bool split7 = dense_backward_data_splits(G.off7, 3) > 1, split5 = dense_backward_data_splits(G.off5, 3) > 1;
    if (bf && split7) zb.add(gh, G.E);     // (gh is written last: free until then)
    if (zb.overflow) return DLKA_ERR_WORKSPACE;
    DLKA_TRY(launch_zero_batch(zb, st));
    float *gxt = gt2;   // (gt2 is dead by the time the last projection's data gradient is written)
    DLKA_TRY(frame_backward_head(G, PW, S, gy_, gyt, gg1, ga1, gt2, st));
    // conv_spatial = DeformConv(7x7 dil 3): t2 = DDW7(t1, o7 = offnet7(t1))
    DwArgs2d d;
    fill_ddw(d, G, 7, 9, 3);
    d.act_bf16 = bf;
    d.in = t1; d.off = o7; d.wp = PW.dw7; d.g = gt2; d.gx = gta; d.goff = goff; d.part = part_dw;
    DLKA_TRY(fork_gx());
    DLKA_TRY(launch_cl_ddw2d_bwd(d, (float *)gr->conv_spatial_w, st, gst));
    DLKA_TRY(fork_to_aux());
    DLKA_TRY(dense_backward_weight(G.off7, t1, goff, 1, (float *)gr->conv_spatial_offset_w, (float *)gr->conv_spatial_offset_b, part_o7, wst, &fb.j[fb.njobs++], 0, pad7));
    DLKA_TRY(join_gx());
    DLKA_TRY(dense_backward_data(G.off7, goff, 1, N0, gt1, PW.o7_b, 3, gta, st, nullptr, nullptr, bf && split7, false, bf != 0, bf ? gh : nullptr));   // gt1 = gta + offnet7^T goff
    // conv0 = DeformConv(5x5): t1 = DDW5(a, o5 = offnet5(a))
    fill_ddw(d, G, 5, 2, 1);
    d.act_bf16 = bf;
    d.in = a; d.off = o5; d.wp = PW.dw5; d.g = gt1; d.gx = gaa; d.goff = goff5; d.part = part_dw;
    DLKA_TRY(fork_gx());
    DLKA_TRY(launch_cl_ddw2d_bwd(d, (float *)gr->conv0_w, st, gst));
    DLKA_TRY(fork_to_aux());
    DLKA_TRY(dense_backward_weight(G.off5, a, goff5, 1, (float *)gr->conv0_offset_w, (float *)gr->conv0_offset_b, part_o5, wst, &fb.j[fb.njobs++], 0, pad5));
    DLKA_TRY(join_gx());
    if (bf && split5) DLKA_TRY(launch_zero(gh, G.E * 4, st));
    DLKA_TRY(dense_backward_data(G.off5, goff5, 1, N0, gab, PW.o5_b, 3, gaa, st, nullptr, nullptr, bf && split5, false, bf != 0, bf ? gh : nullptr));   // gab = gaa + offnet5^T goff
    DLKA_TRY(frame_backward_wgrads(G, S, gr, gyt, gg1, ga1, gab, gh, part_pw, fb, st));
    if (fork2d) DLKA_TRY(lease.join(1));   // the folds read the offset nets' partial sums
    return frame_backward_finish(G, PW, fb, gyt, gh, gxt, gx_, st);
}

}  // namespace dlka
