// C-ABI entry points of the token-layout 3-D D-LKA block (LKA3d_deform inside its attention wrapper) on the channels-last kernels: forward, the one-call and
// the phased backward pass, and the many-block weight-preparation and weight-gradient-finalisation plans.  fp32 and DLKA_BF16 (mixed precision, capi_lka3d_tokens.h).
#include "capi_lka3d_tokens.h"
#include "cl_fork.h"

using namespace dlka;

namespace dlka {

int carve_prep(const TokGeoms &G, float *base, TokPrep &t, const dlka_lka3d_params *p, hipStream_t st, bool fill, const ZeroBatch *zb,
               PrepBatch *collect, bool append)
{
    float *q = base;
    auto take = [&](size_t n) { float *r = q; q += (n + 63) & ~(size_t)63; return r; };
    for (int k = 0; k < 3; ++k) { t.pw_f[k] = take(G.pw_floats()); t.pw_b[k] = take(G.pw_floats()); }
    t.off_f = take(G.offc_floats()); t.off_b = take(G.offc_floats());
    t.dcn_f = take(G.dcn_floats()); t.dcn_b = take(G.dcn_floats());
    t.dw5_f = take(G.dw5_floats()); t.dw5_b = take(G.dw5_floats());
    t.dw7_f = take(G.dw7_floats()); t.dw7_b = take(G.dw7_floats());
    t.dcn_b16 = take(G.dcn_floats());
    if (!fill) return DLKA_OK;
    PrepBatch pb;
    if (collect && append) pb = *collect;
    else memset(&pb, 0, sizeof(pb));
    if (pb.njobs + 15 + (zb ? zb->n : 0) > PREP_MAX_JOBS) return DLKA_ERR_WORKSPACE;
    const int C = G.pw.Cin;
    const void *pw_w[3] = {p->proj_1_w, p->conv1_w, p->proj_2_w};
    for (int k = 0; k < 3; ++k) {
        add_job(pb, pw_w[k], t.pw_f[k], C, C, 1, C, C, 0);
        add_job(pb, pw_w[k], t.pw_b[k], C, C, 1, C, C, 1);
    }
    add_job(pb, p->offset_w, t.off_f, 81, C, 27, C, 96, split_mode_flag(use_split(G.offc_f, true)));   // (fp32 A operand on both paths)
    add_job(pb, p->offset_w, t.off_b, 81, C, 27, 96, C, use_split(G.offc, false) ? 9 : 1);
    add_job(pb, p->deform_w, t.dcn_f, C, C, 27, C, C, (G.dcn.act_bf16 && deform_b16()) ? 8 : 0);   // bf16 path: two-term records for cl_deform_fwd_b16_kernel
    add_job(pb, p->deform_w, t.dcn_b, C, C, 27, C, C, 2);
    if (deform_b16()) add_job(pb, p->deform_w, t.dcn_b16, C, C, 27, C, C, 2 | 8);   // (both dtypes: the backward contractions of the deformable conv)
    add_job(pb, p->conv0_w, t.dw5_f, C, C, G.dw5.K, 0, 0, 3);
    add_job(pb, p->conv0_w, t.dw5_b, C, C, G.dw5.K, 0, 0, 4);
    add_job(pb, p->conv_spatial_w, t.dw7_f, C, C, G.dw7.K, 0, 0, 3);
    add_job(pb, p->conv_spatial_w, t.dw7_b, C, C, G.dw7.K, 0, 0, 4);
    if (zb && pb.njobs + zb->n > PREP_MAX_JOBS) return DLKA_ERR_WORKSPACE;   // (a dropped zero fill would be a silent wrong answer)
    if (zb)   // the forward pass's zero fills ride along (one launch less per block)
        for (int r = 0; r < zb->n; ++r) {
            PrepJob &j = pb.j[pb.njobs++];
            memset(&j, 0, sizeof(j));
            j.dst = zb->p[r]; j.n = zb->cnt[r]; j.mode = 5;
            pb.total += j.n;
        }
    if (collect) { *collect = pb; return DLKA_OK; }   // dlka_lka3d_tokens_prepare_plan: the jobs go into a table instead of a launch
    return launch_cl_prep_batch(pb, st);
}

bool tokens_supported(int B, int C, int D, int H, int W, int variant)
{
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0) return false;
    if (!(C == 32 || C == 64 || C == 128 || C == 256)) return false;
    if ((long)B * D * H * W > (1l << 28)) return false;
    DwPairCfg dc;
    if (!dw_pair_cfg(variant, C, dc)) return false;
    return dw_supported(dw_conv(B, C, D, H, W, dc.k0, dc.p0, dc.d0, 0)) && dw_supported(dw_conv(B, C, D, H, W, dc.k1, dc.p1, dc.d1, 0));
}

}  // namespace dlka

extern "C" {

// ---- token-layout D-LKA block ------------------------------------------------------------------------------------------------
int dlka_lka3d_tokens_supported_v(int B, int C, int D, int H, int W, int dtype, int variant)
{
    return ((dtype == DLKA_F32 || dtype == DLKA_BF16) && tokens_supported(B, C, D, H, W, variant)) ? 1 : 0;
}
int dlka_lka3d_tokens_supported(int B, int C, int D, int H, int W, int dtype) { return dlka_lka3d_tokens_supported_v(B, C, D, H, W, dtype, DLKA_LKA3D_SYNAPSE); }

size_t dlka_lka3d_tokens_saved_bytes_v(int B, int C, int D, int H, int W, int dtype, int variant)
{
    if (!dlka_lka3d_tokens_supported_v(B, C, D, H, W, dtype, variant)) return 0;
    return tok_saved_bytes(TokGeoms(B, C, D, H, W, dtype, variant));
}
size_t dlka_lka3d_tokens_saved_bytes(int B, int C, int D, int H, int W, int dtype) { return dlka_lka3d_tokens_saved_bytes_v(B, C, D, H, W, dtype, DLKA_LKA3D_SYNAPSE); }

size_t dlka_lka3d_tokens_workspace_bytes(int B, int C, int D, int H, int W, int dtype) { return dlka_lka3d_tokens_workspace_bytes_v(B, C, D, H, W, dtype, DLKA_LKA3D_SYNAPSE); }
size_t dlka_lka3d_tokens_workspace_bytes_v(int B, int C, int D, int H, int W, int dtype, int variant)
{
    if (!dlka_lka3d_tokens_supported_v(B, C, D, H, W, dtype, variant)) return 0;
    return tok_workspace_bytes(TokGeoms(B, C, D, H, W, dtype, variant));
}

// x_f32 (DLKA_BF16 only, optional): the caller's UNROUNDED fp32 twin of the bf16 input x.  The chain that decides where the deformable conv samples then starts
// from it (a32 = GELU(proj_1 x_f32) by one extra fp32 pointwise launch) instead of from the bf16 tensor: the wrapper block's mixed mode rounds LayerNorm's output
// INSIDE the block, and 2^-9 of input rounding in front of floor() would flip sampling cells against the fp32 block (tests/parity.py::check_tblock3d_mixed_bf16).
}  // extern "C"

int dlka::tokens_forward_impl(const void *x_, const dlka_lka3d_params *p, void *y_, void *saved, size_t saved_bytes, void *workspace,
                              size_t workspace_bytes, int B, int C, int D, int H, int W, int dtype, void *stream, bool prepared,
                              int variant, const float *x_f32)
{
    if (!x_ || !all_set(p) || !y_ || !saved || !workspace) return DLKA_ERR_NULL;
    if (!dlka_lka3d_tokens_supported_v(B, C, D, H, W, dtype, variant)) return DLKA_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    // DLKA_BF16: x, y and every saved activation are bf16 storage (`float *` below is then just an address: the kernels reinterpret it);
    // offsets, prepared weights, parameters and all accumulators are fp32
    TokGeoms G(B, C, D, H, W, dtype, variant);
    Carver sv(saved, saved_bytes), cv(workspace, workspace_bytes);
    const TokSaved S = carve_tok_saved(sv, G);
    const TokFwdWs Wf = carve_tok_fwd_ws(cv, G);
    if (!sv.ok() || !cv.ok()) return DLKA_ERR_WORKSPACE;
    TokWsTail Wt = {nullptr, nullptr};
    if (deform_fwd_slab_floats(G.dcn)) Wt = carve_tok_ws_tail(cv, G);   // (a workspace without the tail serves every stage that needs no slabs)
    if (!cv.ok()) return DLKA_ERR_WORKSPACE;
    float *h = S.h, *a = S.a, *t1 = S.t1, *t = S.t, *off = S.off, *f = S.f, *g1 = S.g1, *prep = S.prep, *m = S.m;
    float *a32 = Wf.a32, *t1_32 = Wf.t1_32, *t_32 = Wf.t_32, *blkA = Wf.blkA, *blkB = Wf.blkB, *slab = Wt.slab;
    const bool bf = dtype == DLKA_BF16;
    const float *x = (const float *)x_;
    float *y = (float *)y_;
    const float *N0 = nullptr;
    // every weight re-layout of the block (forward and backward forms) in one launch; the backward call reuses them
    // outputs of tap-split convs (small stages) collect partial sums with atomics: their zero fills ride in the weight-preparation launch
    ZeroBatch zb;
    memset(&zb, 0, sizeof(zb));
    if (dense_forward_splits(G.offc_f, 0) > 1) zb.add(off, G.Off);
    if (dense_forward_splits(G.pw, 3) > 1) zb.add(y, G.E);
    TokPrep PW;
    const ZeroBatch *ride = nullptr;
    if (prepared) {   // the prepared weights are already in `saved` (dlka_lka3d_tokens_prepare_run): the zero fills ride in the first kernel
        DLKA_TRY(carve_prep(G, prep, PW, p, st, false));
        if (zb.n) ride = &zb;
    } else {
        DLKA_TRY(carve_prep(G, prep, PW, p, st, true, &zb));
    }
    // proj_1 + GELU (transformerblock.py:667-668): h kept for the GELU gradient, a = GELU(h)   (bf16: + the unrounded a for the fp32 chain)
    if (bf && x_f32) {   // (t_32 is free until the dilated conv writes it: the fp32 pre-activation lands there and is never read)
        DLKA_TRY(dense_forward(G.pw_f, x_f32, N0, (const float *)p->proj_1_b, t_32, 0, PW.pw_f[0], 1, nullptr, a32, st, false, ride));
        ride = nullptr;
        DLKA_TRY(dense_forward(G.pw, x, N0, (const float *)p->proj_1_b, h, 0, PW.pw_f[0], 1, nullptr, a, st));
    } else
        DLKA_TRY(dense_forward(G.pw, x, N0, (const float *)p->proj_1_b, h, 0, PW.pw_f[0], 1, nullptr, a, st, false, ride, bf ? a32 : nullptr));
    // depthwise 5^3 then 7^3 dilation 3 (:646-647)   (bf16: fp32 in / out, the bf16 copies t1 / t ride in the same kernels)
    const float *a_in = bf ? a32 : a;
    float *t1_out = bf ? t1_32 : t1, *t_out = bf ? t_32 : t;
    bool chained = false;
    DwBlk bk5, bk7;
    bk5.blk = blkA; bk5.blk_floats = G.blk_floats(); bk5.chain = &G.dw7_f; bk5.chain_blk = blkB; bk5.chained = &chained;
    const int pair = dw_pair(G.dw5_f, G.dw7_f, a_in, PW.dw5_f, (const float *)p->conv0_b, t1_out, bf ? t1 : nullptr, PW.dw7_f, (const float *)p->conv_spatial_b, t_out,
                             bf ? t : nullptr, nullptr, nullptr, st);   // 8^3 / 4^3 stages: both in one launch
    if (pair != DLKA_ERR_UNSUPPORTED) DLKA_TRY(pair);
    else {
        DLKA_TRY(dw_forward(G.dw5_f, a_in, N0, (const float *)p->conv0_b, t1_out, PW.dw5_f, 0, st, nullptr, nullptr, bf ? t1 : nullptr, &bk5));
        bk7.blk = blkB; bk7.blk_floats = G.blk_floats(); bk7.in_blocked = chained;
        DLKA_TRY(dw_forward(G.dw7_f, t1_out, N0, (const float *)p->conv_spatial_b, t_out, PW.dw7_f, 0, st, nullptr, nullptr, bf ? t : nullptr, &bk7));
    }
    // offset-predict conv C -> 81 (synapse/deform_conv.py:94) on the fp32 t; offsets stay in the reference's planar layout
    DLKA_TRY(dense_forward(G.offc_f, t_out, N0, (const float *)p->offset_b, off, 1, PW.off_f, 0, nullptr, nullptr, st, true));
    // deformable 3^3 conv (deform_conv.py:95-105)   (bf16: samples the bf16 copy of t)
    DLKA_TRY(deform_forward(G.dcn, t, off, N0, (const float *)p->deform_b, f, PW.dcn_f, st, slab));
    // conv1 + gate u*attn (:650-652): g1 kept, m = a * g1
    // ... and proj_2 + shortcut (:670-671) — one launch at C <= 64 (cl_pointwise_pair_kernel)
    const int prc = pointwise_pair(G.pw, 0, f, PW.pw_f[1], (const float *)p->conv1_b, PW.pw_f[2], (const float *)p->proj_2_b, a, x, g1, m, y, st);
    if (prc != DLKA_ERR_UNSUPPORTED) return prc;
    DLKA_TRY(dense_forward(G.pw, f, N0, (const float *)p->conv1_b, g1, 0, PW.pw_f[1], 2, a, m, st));
    DLKA_TRY(dense_forward(G.pw, m, N0, (const float *)p->proj_2_b, y, 0, PW.pw_f[2], 3, x, nullptr, st, true));
    return DLKA_OK;
}

extern "C" {

int dlka_lka3d_attention_tokens_forward(const void *x, const dlka_lka3d_params *p, void *y, void *saved, size_t saved_bytes, void *workspace,
                                        size_t workspace_bytes, int B, int C, int D, int H, int W, int dtype, void *stream)
{
    return tokens_forward_impl(x, p, y, saved, saved_bytes, workspace, workspace_bytes, B, C, D, H, W, dtype, stream, false);
}

int dlka_lka3d_attention_tokens_forward_v(const void *x, const dlka_lka3d_params *p, void *y, void *saved, size_t saved_bytes, void *workspace,
                                          size_t workspace_bytes, int B, int C, int D, int H, int W, int dtype, int variant, void *stream)
{
    return tokens_forward_impl(x, p, y, saved, saved_bytes, workspace, workspace_bytes, B, C, D, H, W, dtype, stream, false, variant);
}

int dlka_lka3d_attention_tokens_forward_prepared(const void *x, const dlka_lka3d_params *p, void *y, void *saved, size_t saved_bytes, void *workspace,
                                                 size_t workspace_bytes, int B, int C, int D, int H, int W, int dtype, void *stream)
{
    return tokens_forward_impl(x, p, y, saved, saved_bytes, workspace, workspace_bytes, B, C, D, H, W, dtype, stream, true);
}

// ---- weight preparation of MANY blocks in one launch --------------------------------------------------------------------------------
// plan (host, then copied to the device by the caller): [header][int first[MAXJ + 1]: first workgroup of job j][int blkjob[nblocks + 1]: first job of block k][PrepJob jobs[MAXJ]]
namespace {
constexpr int PLAN_JOBS_PER_BLOCK = 16;   // (14 today: 6 pointwise, 2 offset conv, 2 deformable, 4 depthwise forms)
struct PlanHeader { int njobs, nblocks, pad0, pad1; };
size_t plan_first_off() { return sizeof(PlanHeader); }
size_t plan_blkjob_off(int nb) { return sizeof(PlanHeader) + ((size_t)nb * PLAN_JOBS_PER_BLOCK + 1) * sizeof(int); }
size_t plan_jobs_off(int nb) { return align256(plan_blkjob_off(nb) + (size_t)(nb + 1) * sizeof(int)); }
}  // namespace

size_t dlka_lka3d_tokens_prepare_plan_bytes(int nblocks)
{
    if (nblocks <= 0) return 0;
    return plan_jobs_off(nblocks) + (size_t)nblocks * PLAN_JOBS_PER_BLOCK * sizeof(PrepJob);
}

int dlka_lka3d_tokens_prepare_plan(int nblocks, const dlka_lka3d_params *params, void *const *saved, const size_t *saved_bytes, const int *dims5,
                                   int dtype, void *plan_host, size_t plan_bytes)
{
    if (!params || !saved || !saved_bytes || !dims5 || !plan_host) return DLKA_ERR_NULL;
    if (nblocks <= 0 || plan_bytes < dlka_lka3d_tokens_prepare_plan_bytes(nblocks)) return DLKA_ERR_WORKSPACE;
    unsigned char *base = (unsigned char *)plan_host;
    PlanHeader *hd = (PlanHeader *)base;
    int *first = (int *)(base + plan_first_off());
    PrepJob *jobs = (PrepJob *)(base + plan_jobs_off(nblocks));
    int *blkjob = (int *)(base + plan_blkjob_off(nblocks));
    int nj = 0, nb = 0;
    for (int k = 0; k < nblocks; ++k) {
        blkjob[k] = nj;
        const int B = dims5[5 * k], C = dims5[5 * k + 1], D = dims5[5 * k + 2], H = dims5[5 * k + 3], W = dims5[5 * k + 4];
        if (!dlka_lka3d_tokens_supported(B, C, D, H, W, dtype)) return DLKA_ERR_UNSUPPORTED;
        TokGeoms G(B, C, D, H, W, dtype);
        Carver sv(saved[k], saved_bytes[k]);
        const TokSaved S = carve_tok_saved(sv, G);
        if (!S.prep) return DLKA_ERR_WORKSPACE;   // (the plan writes the prepared weights only: a buffer that ends behind them will do)
        TokPrep PW;
        PrepBatch pb;
        DLKA_TRY(carve_prep(G, S.prep, PW, &params[k], nullptr, true, nullptr, &pb));
        if (pb.njobs > PLAN_JOBS_PER_BLOCK) return DLKA_ERR_UNSUPPORTED;
        for (int j = 0; j < pb.njobs; ++j) {
            first[nj] = nb;
            jobs[nj] = pb.j[j];
            nb += cl_prep_table_blocks(pb.j[j]);
            ++nj;
        }
    }
    blkjob[nblocks] = nj;
    first[nj] = nb;   // (end marker: the workgroups of job j are first[j] .. first[j + 1])
    hd->njobs = nj; hd->nblocks = nb; hd->pad0 = hd->pad1 = 0;
    return DLKA_OK;
}

int dlka_lka3d_tokens_prepare_run_range(const void *plan_device, const void *plan_host, int nblocks, int block_lo, int block_hi, void *stream)
{
    if (!plan_device || !plan_host) return DLKA_ERR_NULL;
    if (block_lo < 0 || block_hi > nblocks || block_lo >= block_hi) return DLKA_ERR_SHAPE;
    const unsigned char *hst = (const unsigned char *)plan_host;   // (the counts are read from the host copy: no device round trip)
    const int *first = (const int *)(hst + plan_first_off()), *blkjob = (const int *)(hst + plan_blkjob_off(nblocks));
    const int jlo = blkjob[block_lo], jhi = blkjob[block_hi];
    const unsigned char *dev = (const unsigned char *)plan_device;
    return launch_cl_prep_table((const PrepJob *)(dev + plan_jobs_off(nblocks)), (const int *)(dev + plan_first_off()), jlo, jhi, first[jhi] - first[jlo],
                                (hipStream_t)stream);
}

int dlka_lka3d_tokens_prepare_run(const void *plan_device, const void *plan_host, int nblocks, void *stream)
{
    return dlka_lka3d_tokens_prepare_run_range(plan_device, plan_host, nblocks, 0, nblocks, stream);
}

int dlka_lka3d_attention_tokens_backward(const void *x_, const dlka_lka3d_params *p, const void *gy_, const void *saved, size_t saved_bytes,
                                         void *gx_, const dlka_lka3d_grads *gr, void *workspace, size_t workspace_bytes, int B, int C,
                                         int D, int H, int W, int dtype, void *stream)
{
    return dlka_lka3d_attention_tokens_backward_v(x_, p, gy_, saved, saved_bytes, gx_, gr, workspace, workspace_bytes, B, C, D, H, W, dtype, DLKA_LKA3D_SYNAPSE, stream);
}

// ---- weight-gradient finalisation of MANY blocks in one launch (include/dlka.h: dlka_wgrad_finalize_*) --------------------------------
// plan (host; the caller copies it to the device once): [FinPlanHeader][int first_job[nblocks + 1]][FinalizeJob jobs[FIN_JOBS_PER_BLOCK * nblocks]]
// jobs are stored block after block (block k: first_job[k] .. first_job[k + 1]), block0 = running workgroup count.
namespace {
struct FinPlanHeader { int nblocks, sealed, pad0, pad1; long total_blocks; long pad2; };
size_t fin_first_off() { return sizeof(FinPlanHeader); }
size_t fin_jobs_off(int nb) { return align256(sizeof(FinPlanHeader) + (size_t)(nb + 1) * sizeof(int)); }
}  // namespace

size_t dlka_lka3d_tokens_partials_bytes_v(int B, int C, int D, int H, int W, int dtype, int variant)
{
    if (!dlka_lka3d_tokens_supported_v(B, C, D, H, W, dtype, variant)) return 0;
    return TokGeoms(B, C, D, H, W, dtype, variant).part_bytes;
}

size_t dlka_wgrad_finalize_plan_bytes(int nblocks)
{
    if (nblocks <= 0) return 0;
    return fin_jobs_off(nblocks) + (size_t)nblocks * FIN_JOBS_PER_BLOCK * sizeof(FinalizeJob);
}

int dlka_wgrad_finalize_plan_init(void *plan_host, size_t plan_bytes, int nblocks)
{
    if (!plan_host) return DLKA_ERR_NULL;
    if (nblocks <= 0 || plan_bytes < dlka_wgrad_finalize_plan_bytes(nblocks)) return DLKA_ERR_WORKSPACE;
    memset(plan_host, 0, dlka_wgrad_finalize_plan_bytes(nblocks));
    ((FinPlanHeader *)plan_host)->nblocks = nblocks;
    return DLKA_OK;
}

int dlka_lka3d_attention_tokens_backward_deferred_v(const void *x, const dlka_lka3d_params *p, const void *grad_y, const void *saved, size_t saved_bytes,
                                                    void *grad_x, const dlka_lka3d_grads *grads, void *workspace, size_t workspace_bytes, void *partials,
                                                    size_t partials_bytes, void *plan_host, int plan_slot, int B, int C, int D, int H, int W, int dtype,
                                                    int variant, void *stream)
{
    if (!partials) return DLKA_ERR_NULL;
    FinalizeJob jobs[FIN_JOBS_PER_BLOCK];
    int nj = 0;
    DLKA_TRY(tokens_backward_impl(x, p, grad_y, saved, saved_bytes, grad_x, grads, workspace, workspace_bytes, B, C, D, H, W, dtype, variant, stream, partials,
                                  partials_bytes, jobs, &nj));
    if (plan_host) {   // record this block's jobs (slots must be filled in ascending order, every slot once, before _plan_seal)
        FinPlanHeader *hd = (FinPlanHeader *)plan_host;
        if (plan_slot < 0 || plan_slot >= hd->nblocks || hd->sealed) return DLKA_ERR_SHAPE;
        int *first = (int *)((unsigned char *)plan_host + fin_first_off());
        FinalizeJob *all = (FinalizeJob *)((unsigned char *)plan_host + fin_jobs_off(hd->nblocks));
        // slots may be recorded in any order: block k owns the fixed window [k * FIN_JOBS_PER_BLOCK, ..); sealing compacts them
        for (int j = 0; j < nj; ++j) all[plan_slot * FIN_JOBS_PER_BLOCK + j] = jobs[j];
        first[plan_slot] = nj;   // (count until sealed)
    }
    return DLKA_OK;
}

int dlka_lka3d_attention_tokens_backward_phase_v(const void *x, const dlka_lka3d_params *p, const void *grad_y, const void *saved, size_t saved_bytes,
                                                 void *grad_x, const dlka_lka3d_grads *grads, void *workspace, size_t workspace_bytes, void *partials,
                                                 size_t partials_bytes, void *plan_host, int plan_slot, int phase, int B, int C, int D, int H, int W, int dtype,
                                                 int variant, void *stream)
{
    if (!partials) return DLKA_ERR_NULL;
    if (phase != 1 && phase != 2) return DLKA_ERR_SHAPE;
    FinalizeJob jobs[FIN_JOBS_PER_BLOCK];
    int nj = 0;
    DLKA_TRY(tokens_backward_impl(x, p, grad_y, saved, saved_bytes, grad_x, grads, workspace, workspace_bytes, B, C, D, H, W, dtype, variant, stream, partials,
                                  partials_bytes, jobs, &nj, phase));
    if (plan_host && phase == 2) {
        FinPlanHeader *hd = (FinPlanHeader *)plan_host;
        if (plan_slot < 0 || plan_slot >= hd->nblocks || hd->sealed) return DLKA_ERR_SHAPE;
        int *first = (int *)((unsigned char *)plan_host + fin_first_off());
        FinalizeJob *all = (FinalizeJob *)((unsigned char *)plan_host + fin_jobs_off(hd->nblocks));
        for (int j = 0; j < nj; ++j) all[plan_slot * FIN_JOBS_PER_BLOCK + j] = jobs[j];
        first[plan_slot] = nj;
    }
    return DLKA_OK;
}

int dlka_wgrad_finalize_run_slot(const void *plan_host, int plan_slot, void *stream)
{
    if (!plan_host) return DLKA_ERR_NULL;
    const FinPlanHeader *hd = (const FinPlanHeader *)plan_host;
    if (hd->sealed || plan_slot < 0 || plan_slot >= hd->nblocks) return DLKA_ERR_SHAPE;
    const int *first = (const int *)((const unsigned char *)plan_host + fin_first_off());
    const FinalizeJob *all = (const FinalizeJob *)((const unsigned char *)plan_host + fin_jobs_off(hd->nblocks));
    const int cnt = first[plan_slot];
    if (cnt <= 0 || cnt > FIN_JOBS_PER_BLOCK) return DLKA_ERR_SHAPE;
    FinalizeBatch fb;
    memset(&fb, 0, sizeof(fb));
    for (int j = 0; j < cnt; ++j) fb.j[j] = all[plan_slot * FIN_JOBS_PER_BLOCK + j];
    fb.njobs = cnt;
    return launch_cl_wgrad_finalize(fb, (hipStream_t)stream);
}

int dlka_wgrad_finalize_plan_seal(void *plan_host)
{
    if (!plan_host) return DLKA_ERR_NULL;
    FinPlanHeader *hd = (FinPlanHeader *)plan_host;
    if (hd->sealed) return DLKA_OK;
    const int nb = hd->nblocks;
    int *first = (int *)((unsigned char *)plan_host + fin_first_off());
    FinalizeJob *all = (FinalizeJob *)((unsigned char *)plan_host + fin_jobs_off(nb));
    int nj = 0;
    long blk = 0;
    for (int k = 0; k < nb; ++k) {
        const int cnt = first[k];
        if (cnt <= 0 || cnt > FIN_JOBS_PER_BLOCK) return DLKA_ERR_SHAPE;   // a slot was never recorded
        first[k] = nj;
        for (int j = 0; j < cnt; ++j) {
            FinalizeJob jb = all[k * FIN_JOBS_PER_BLOCK + j];
            jb.block0 = blk;
            blk += cl_wgrad_finalize_plan_job(jb);
            all[nj++] = jb;   // (nj <= k * FIN_JOBS_PER_BLOCK + j: compaction never overtakes the reads)
        }
    }
    first[nb] = nj;
    hd->total_blocks = blk;
    hd->sealed = 1;
    return DLKA_OK;
}

int dlka_wgrad_finalize_run(const void *plan_device, const void *plan_host, int block_lo, int block_hi, void *stream)
{
    if (!plan_device || !plan_host) return DLKA_ERR_NULL;
    const FinPlanHeader *hd = (const FinPlanHeader *)plan_host;   // (counts are read from the host copy: no device round trip)
    if (!hd->sealed || block_lo < 0 || block_hi > hd->nblocks || block_lo >= block_hi) return DLKA_ERR_SHAPE;
    const int *first = (const int *)((const unsigned char *)plan_host + fin_first_off());
    const FinalizeJob *all_h = (const FinalizeJob *)((const unsigned char *)plan_host + fin_jobs_off(hd->nblocks));
    const int jlo = first[block_lo], jhi = first[block_hi];
    const long b_lo = all_h[jlo].block0;
    const long b_hi = block_hi == hd->nblocks ? hd->total_blocks : all_h[jhi].block0;
    const FinalizeJob *all_d = (const FinalizeJob *)((const unsigned char *)plan_device + fin_jobs_off(hd->nblocks));
    return launch_cl_wgrad_finalize_table(all_d, jlo, jhi, b_hi - b_lo, (hipStream_t)stream);
}

int dlka_lka3d_attention_tokens_backward_v(const void *x_, const dlka_lka3d_params *p, const void *gy_, const void *saved, size_t saved_bytes,
                                           void *gx_, const dlka_lka3d_grads *gr, void *workspace, size_t workspace_bytes, int B, int C,
                                           int D, int H, int W, int dtype, int variant, void *stream)
{
    return tokens_backward_impl(x_, p, gy_, saved, saved_bytes, gx_, gr, workspace, workspace_bytes, B, C, D, H, W, dtype, variant, stream, nullptr, 0, nullptr,
                                nullptr);
}

}  // extern "C"

// partials != nullptr: the weight gradients' partial sums go to that (block-private) area and the finalisation is NOT launched — its jobs are
// returned in jobs_out / njobs_out for dlka_wgrad_finalize_run
int dlka::tokens_backward_impl(const void *x_, const dlka_lka3d_params *p, const void *gy_, const void *saved, size_t saved_bytes, void *gx_,
                         const dlka_lka3d_grads *gr, void *workspace, size_t workspace_bytes, int B, int C, int D, int H, int W, int dtype, int variant,
                         void *stream, void *partials, size_t partials_bytes, FinalizeJob *jobs_out, int *njobs_out, int phase, const FinalizeBatch *extra)
{
    if (!x_ || !p || !gy_ || !saved || !gx_ || !gr || !workspace) return DLKA_ERR_NULL;
    if (phase < 0 || phase > 2) return DLKA_ERR_SHAPE;
    if (!all_set(p) || !all_set(gr)) return DLKA_ERR_NULL;
    if (!dlka_lka3d_tokens_supported_v(B, C, D, H, W, dtype, variant)) return DLKA_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    // DLKA_BF16: x, gy, gx, the saved activations and the intermediate gradients gg1, ga1, gf, gt, gt1, gh are bf16 storage; grad_offset, the
    // deformable conv's grad_input accumulator gta (atomics), the weight-gradient partials and the parameter gradients are fp32
    TokGeoms G(B, C, D, H, W, dtype, variant);
    const bool bf = dtype == DLKA_BF16;
    Carver sv(saved, saved_bytes), cv(workspace, workspace_bytes);
    const TokSaved S = carve_tok_saved(sv, G);   // (written by the matching forward call)
    const TokBwdWs Wb = carve_tok_bwd_ws(cv, G);
    if (!sv.ok() || !cv.ok()) return DLKA_ERR_WORKSPACE;
    Carver pc(partials ? partials : Wb.part, partials ? partials_bytes : G.part_bytes);
    const TokPartials P = G.carve_partials(pc);
    if (!pc.ok()) return DLKA_ERR_WORKSPACE;
    const float *h = S.h, *a = S.a, *t1 = S.t1, *t = S.t, *off = S.off, *f = S.f, *g1 = S.g1, *m = S.m;
    float *prep = S.prep;
    float *gg1 = Wb.gg1, *ga1 = Wb.ga1, *gf = Wb.gf, *gta = Wb.gta, *gt = Wb.gt, *gt1 = Wb.gt1, *ga2 = Wb.ga2, *gh = Wb.gh;
    float *goff = Wb.goff, *scratch = Wb.scratch, *blkA = Wb.blkA, *blkB = Wb.blkB, *padt = Wb.padt;
    float *samp = wgrad_gather() ? nullptr : Wb.samp;   // (the switch is read once here)
    const float *x = (const float *)x_, *gy = (const float *)gy_;
    float *gx = (float *)gx_;
    const float *N0 = nullptr;
    TokPrep PW;
    DLKA_TRY(carve_prep(G, prep, PW, p, st, false));
    // partial-sum areas, one per weight gradient; folded by ONE launch at the end
    float *part_p2 = P.p2, *part_c1 = P.c1, *part_p1 = P.p1, *part_off = P.off, *part_dcn = P.dcn, *stage5 = P.stage5, *stage7 = P.stage7;
    FinalizeBatch fb;
    memset(&fb, 0, sizeof(fb));

    // one lease for the call: `s` for grad_input beside grad_offset
    const bool want_gx_fork = phase != 2 && gx_fork_wanted((long)G.dcn.M, phase);
    ForkLease lease(st, want_gx_fork);
    // everything that is accumulated into with atomics, zero-filled by ONE launch: the depthwise weight-gradient staging, the
    // deformable conv's grad_input (halo overflow of the LDS windows) and the outputs of tap-split data gradients
    ZeroBatch zb;
    memset(&zb, 0, sizeof(zb));
    zb.add(stage5, G.stage_dw());
    zb.add(gta, G.E);
    // grad_offset has ONE producer and two 27-tap consumers that contract it on the bf16 matrix cores (offset conv data / weight gradient):
    // the producer stores it already split (pack_split2 words, 96 channel planes) unless its channel-sliced variant needs fp32 atomics
    int goff_cpad = 0;
    {
        DeformBwdArgs da;
        fill_deform_bwd(da, G.dcn);
        // Measured with the workgroup-tiled consumers (profiles/archive/r01v): no gain — they are bound by per-unit latency (barrier + staging per
        // 192 MFMA cycles), not by the split arithmetic (grad_offset +14 us, weight gradient +18 us, data gradient unchanged at 32^3) — so the
        // packed hand-over is opt-in (DLKA_GOFF_PACKED=1) until the consumers are wave-granular.
        const bool fp32_goff = bf || getenv("DLKA_GOFF_PACKED") == nullptr;   // (not cached: tests toggle it)
        const bool sliced = cl_deform_goff_ccsplit(da) > 1;
        if (sliced) zb.add(goff, G.Off);
        // (N % 16: the weight-gradient kernel's split variant exists for 16-voxel-aligned volumes only, cl_wgrad.hip)
        else if (!fp32_goff && use_split(G.offc, false) == 2 && (G.offc.N & 15) == 0) goff_cpad = 96;
    }
    if (dense_backward_data_splits(G.pw, 0) > 1) zb.add(gf, G.E);
    if (dense_backward_data_splits(G.offc, 3) > 1) zb.add(bf ? ga2 : gt, G.E);   // bf16: split partial sums land in the fp32 scratch ga2
    if (dense_backward_data_splits(G.pw, 3) > 1) zb.add(gx, G.E);
    // the word the half hand-over's max |t| is accumulated into (fp32 path; cl_absmax_bits_kernel): zeroed with the rest instead of by a launch of its own
    float *samp_max = (samp && !bf) ? samp + (size_t)G.dcn.K * G.dcn.M * G.dcn.Cin / 2 : nullptr;
    zb.add(samp_max, 1);
    if (zb.overflow) return DLKA_ERR_WORKSPACE;
    // (the zero fills ride in the first kernel below: one dependent node less per block)

    // proj_2:  y = P2 m + x.   Its data gradient gm = P2^T gy feeds only the gate  m = a * g1, whose backward is fused into
    // the epilogue:  gg1 = gm * a,  ga1 = gm * g1
    // (the three pointwise weight gradients run as ONE launch at the end: their operands m/gy, f/gg1, x/gh all stay live)
    // ... and conv1:  g1 = P0 f,  gf = P0^T gg1 — one launch at C <= 64
    // phase: 0 = the whole backward pass; 1 = the DATA-gradient chain only (everything the next block needs: gx; and what the weight gradients read:
    // the intermediate gradients and the stored samples, all in `workspace`); 2 = the five WEIGHT-gradient launches only, reading those — a caller that
    // runs phase 2 on another stream lets them overlap the next block's data chain (DLKABlockStack: two alternating workspaces).
#define DLKA_P1(call) do { if (phase != 2) DLKA_TRY(call); } while (0)
#define DLKA_P2(call) do { if (phase != 1) DLKA_TRY(call); } while (0)
    if (phase != 2) {
        const int prc = dense_backward_data_splits(G.pw, 0) > 1 ? DLKA_ERR_UNSUPPORTED
                                                                : pointwise_pair(G.pw, 1, gy, PW.pw_b[2], nullptr, PW.pw_b[1], nullptr, a, g1, gg1, ga1, gf, st, &zb);
        if (prc != DLKA_ERR_UNSUPPORTED) DLKA_TRY(prc);
        else {
            DLKA_TRY(dense_backward_data(G.pw, gy, 0, N0, gg1, PW.pw_b[2], 4, a, st, g1, ga1, false, false, false, nullptr, &zb));
            DLKA_TRY(dense_backward_data(G.pw, gg1, 0, N0, gf, PW.pw_b[1], 0, nullptr, st, nullptr, nullptr, true));
        }
    }
    // deformable conv:  f = DCN(t, off):  grad_offset, grad_input and the weight gradient — the last one after
    // grad_offset when that kernel hands over the samples it interpolated (samp), else at once with its own gather
    if (!samp)
        DLKA_P2(deform_backward(G.dcn, t, off, N0, gf, nullptr, nullptr, (float *)gr->deform_w, (float *)gr->deform_b, PW.dcn_b, part_dcn, scratch, st,
                                &fb.j[fb.njobs++]));
    bool gx_forked = false;
    if (want_gx_fork && lease.ok()) {   // grad_input on the internal stream, beside grad_offset (see ForkCtx)
        DLKA_TRY(lease.fork(1));
        DLKA_TRY(deform_backward(G.dcn, t, off, N0, gf, gta, nullptr, nullptr, nullptr, PW.dcn_b, nullptr, scratch, lease.stream(1), nullptr, true, false, 0, nullptr, PW.dcn_b16));
        gx_forked = true;
    }
    DLKA_P1(deform_backward(G.dcn, t, off, N0, gf, nullptr, goff, nullptr, nullptr, PW.dcn_b, nullptr, scratch, st, nullptr, false, true, goff_cpad, samp, PW.dcn_b16, samp_max != nullptr));
    if (samp)
        DLKA_P2(deform_backward(G.dcn, t, off, N0, gf, nullptr, nullptr, (float *)gr->deform_w, (float *)gr->deform_b, PW.dcn_b, part_dcn, scratch, st,
                                &fb.j[fb.njobs++], false, false, 0, samp));
    // offset-predict conv:  off = Coff t      (gt = gt_a + Coff^T goff fused in the epilogue)
    DLKA_P2(dense_backward_weight(G.offc, t, goff, 1, (float *)gr->offset_w, (float *)gr->offset_b, part_off, st, &fb.j[fb.njobs++], goff_cpad, padt));
    if (gx_forked) DLKA_TRY(lease.join(1));   // the offset conv's data gradient adds gta
    else
        DLKA_P1(deform_backward(G.dcn, t, off, N0, gf, gta, nullptr, nullptr, nullptr, PW.dcn_b, nullptr, scratch, st, nullptr, true, false, 0, nullptr, PW.dcn_b16));
    DLKA_P1(dense_backward_data(G.offc, goff, 1, N0, gt, PW.off_b, 3, gta, st, nullptr, nullptr, true, goff_cpad != 0, true, ga2));
    // depthwise 7^3 dil 3:  t = DW7 t1
    DLKA_P2(dw_backward_weight(G.dw7, t1, gt, (float *)gr->conv_spatial_w, (float *)gr->conv_spatial_b, stage7, st, &fb.j[fb.njobs++]));
    bool chained = false;
    DwBlk bk7, bk5;
    bk7.blk = blkA; bk7.blk_floats = G.blk_floats(); bk7.chain = &G.dw5; bk7.chain_blk = blkB; bk7.chained = &chained;
    // (8^3 / 4^3 stages: this conv's and the next one's data gradients, GELU' included, in one launch)
    int pair = DLKA_ERR_UNSUPPORTED;
    if (phase != 2) pair = dw_pair(G.dw7, G.dw5, gt, PW.dw7_b, nullptr, gt1, nullptr, PW.dw5_b, nullptr, gh, nullptr, h, ga1, st);
    if (pair != DLKA_ERR_UNSUPPORTED) DLKA_TRY(pair);
    else DLKA_P1(dw_forward(G.dw7, gt, N0, nullptr, gt1, PW.dw7_b, 1, st, nullptr, nullptr, nullptr, &bk7));
    // depthwise 5^3:  t1 = DW5 a
    DLKA_P2(dw_backward_weight(G.dw5, a, gt1, (float *)gr->conv0_w, (float *)gr->conv0_b, stage5, st, &fb.j[fb.njobs++]));
    // ... with the GELU backward in its epilogue:  a = GELU(h),  gh = (ga1 + DW5^T gt1) * gelu'(h)
    bk5.blk = blkB; bk5.blk_floats = G.blk_floats(); bk5.in_blocked = chained;
    if (pair == DLKA_ERR_UNSUPPORTED) DLKA_P1(dw_forward(G.dw5, gt1, N0, nullptr, gh, PW.dw5_b, 1, st, h, ga1, nullptr, &bk5));
    // proj_1:  h = P1 x ;  gx = P1^T gh + gy (shortcut)
    if (phase != 1) {
        WgradArgs jobs[3];
        fill_pw_wgrad(jobs[0], G.pw, m, gy, part_p2);
        fill_pw_wgrad(jobs[1], G.pw, f, gg1, part_c1);
        fill_pw_wgrad(jobs[2], G.pw, x, gh, part_p1);
        float *const gws[3] = {(float *)gr->proj_2_w, (float *)gr->conv1_w, (float *)gr->proj_1_w};
        float *const gbs[3] = {(float *)gr->proj_2_b, (float *)gr->conv1_b, (float *)gr->proj_1_b};
        DLKA_TRY(launch_cl_wgrad_pw3(jobs, gws, gbs, st, &fb.j[fb.njobs]));
        fb.njobs += 3;
    }
    if (partials) {
        if (fb.njobs > FIN_JOBS_PER_BLOCK || !jobs_out || !njobs_out) return DLKA_ERR_UNSUPPORTED;
        for (int k = 0; k < fb.njobs; ++k) jobs_out[k] = fb.j[k];
        *njobs_out = fb.njobs;
    } else {
        if (phase != 0) return DLKA_ERR_UNSUPPORTED;   // the split passes need the deferred finalisation (block-private partial sums)
        if (extra) {   // the caller's own folds (the wrapper block's three conv weight gradients) ride in this launch
            if (fb.njobs + extra->njobs > (int)(sizeof(fb.j) / sizeof(fb.j[0]))) return DLKA_ERR_UNSUPPORTED;
            for (int k = 0; k < extra->njobs; ++k) fb.j[fb.njobs++] = extra->j[k];
        }
        DLKA_TRY(launch_cl_wgrad_finalize(fb, st));
    }
    DLKA_P1(dense_backward_data(G.pw, gh, 0, N0, gx, PW.pw_b[0], 3, gy, st, nullptr, nullptr, true));
#undef DLKA_P1
#undef DLKA_P2
    return DLKA_OK;
}

extern "C" {

int dlka_lka3d_tokens_saved_offsets_v(int B, int C, int D, int H, int W, int dtype, int variant, size_t *byte_offset)
{
    if (!byte_offset) return DLKA_ERR_NULL;
    if (!dlka_lka3d_tokens_supported_v(B, C, D, H, W, dtype, variant)) return DLKA_ERR_UNSUPPORTED;
    Carver sv = Carver::probing();
    *byte_offset = sv.offset_of(carve_tok_saved(sv, TokGeoms(B, C, D, H, W, dtype, variant)).off);
    return DLKA_OK;
}

}  // extern "C"
