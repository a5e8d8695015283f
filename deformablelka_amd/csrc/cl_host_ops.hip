// Per-operator host drivers of the channels-last fast path: each fills the argument record of one kernel family (cl_*.hip) from a SameConv and launches it.
// Also the home of the process-wide switches these drivers read (ONE instance per library: see cl_host.h).
// Everything here is fp32 or bf16 storage as SameConv::act_bf16 says; shapes a driver does not cover return DLKA_ERR_UNSUPPORTED.
#include <atomic>
#include <mutex>

#include "cl_host.h"

namespace dlka {

int make_same_conv(const dlka_conv_geom *c, SameConv &s)
{
    if (!c) return DLKA_ERR_NULL;
    if (c->B <= 0 || c->C <= 0 || c->D <= 0 || c->H <= 0 || c->W <= 0 || c->Cout <= 0) return DLKA_ERR_SHAPE;
    if (c->kd <= 0 || c->kh <= 0 || c->kw <= 0 || c->dd <= 0 || c->dh <= 0 || c->dw <= 0) return DLKA_ERR_SHAPE;
    if (c->group <= 0 || c->C % c->group || c->Cout % c->group) return DLKA_ERR_GROUP;
    if (c->sd != 1 || c->sh != 1 || c->sw != 1) return DLKA_ERR_UNSUPPORTED;
    if (dlka_conv_out_size(c->D, c->pd, c->dd, c->kd, 1) != c->D || dlka_conv_out_size(c->H, c->ph, c->dh, c->kh, 1) != c->H ||
        dlka_conv_out_size(c->W, c->pw, c->dw, c->kw, 1) != c->W)
        return DLKA_ERR_UNSUPPORTED;
    const long N = (long)c->D * c->H * c->W;
    if (N > (1l << 30) || (long)c->B * N > (1l << 30)) return DLKA_ERR_SHAPE;
    s.B = c->B; s.D = c->D; s.H = c->H; s.W = c->W; s.N = (int)N; s.M = (int)(c->B * N);
    s.Cin = c->C; s.Cout = c->Cout; s.group = c->group;
    s.kd = c->kd; s.kh = c->kh; s.kw = c->kw; s.pd = c->pd; s.ph = c->ph; s.pw = c->pw;
    s.dd = c->dd; s.dh = c->dh; s.dw = c->dw; s.K = c->kd * c->kh * c->kw;
    s.act_bf16 = 0;
    return DLKA_OK;
}

bool nt_ok(int np) { const int nt = np / 32; return nt == 1 || nt == 2 || nt == 3 || nt == 4 || nt == 8; }
bool is_depthwise(const SameConv &s) { return s.group == s.Cin && s.Cin == s.Cout; }
bool dw_supported(const SameConv &s)
{
    const bool kshape = (s.kw == 5 && s.dw == 1) || (s.kw == 7 && s.dw == 3) || (s.kw == 3 && s.dw == 1) || (s.kw == 5 && s.dw == 3) ||
                        (s.kw == 7 && s.dw == 1);
    const int cpb = s.Cin < 256 ? s.Cin : 256;
    return kshape && s.Cin % 32 == 0 && 256 % cpb == 0 && s.Cin % cpb == 0;
}
bool dense_fwd_supported(const SameConv &s) { return s.group == 1 && s.Cin % 32 == 0 && nt_ok(round_up(s.Cout, 32)); }

// Contractions with K > 1 taps (the offset-predict conv, its data gradient and its weight gradient) are MFMA-bound with fp32
// inputs; they run on the bf16 matrix cores with split operands and fp32 accumulation (cl_igemm.hip) unless DLKA_EXACT_FP32=1.
// Returns the number of bf16 terms per operand (0 = exact fp32-input MFMA):
//   gradient contractions: 2 (three products, ~1e-5 relative);
//   FORWARD offset conv:   3 (six products, fp32-equivalent).  Its output decides floor() of every sampling position: a 1e-5
//     perturbation flips the cell of the samples that sit within 1e-5 of an integer, and each flip changes that sample's
//     grad_offset by O(1) (seen as 1.5e-2 on conv_offset.weight.grad with offsets concentrated near 0), so the two-term split is
//     not used there by default; DLKA_SPLIT_FORWARD=2 forces it for A/B runs;
//   bf16 activations (DLKA_BF16): the activation is its own high term, weights are split in two, no a_lo products.
int use_split(const SameConv &s, bool forward)
{
    static const bool exact = getenv("DLKA_EXACT_FP32") != nullptr;
    static const int fwd = getenv("DLKA_SPLIT_FORWARD") ? atoi(getenv("DLKA_SPLIT_FORWARD")) : 3;
    if (s.act_bf16) return s.K > 1 ? 2 : 0;   // bf16 activations are their own high term: two-term weights, no a_lo products (cl_igemm.hip)
    if (exact || s.K <= 1) return 0;
    if (!forward) return 2;
    return (fwd == 2 || fwd == 3) ? fwd : 0;
}

// the volume, the kernel / padding / dilation triples and the tap count of `s` into a kernel's argument record (IgemmArgs, WgradArgs, DeformBwdArgs)
template <class Args> static void copy_geom(Args &a, const SameConv &s)
{
    a.B = s.B; a.D = s.D; a.H = s.H; a.W = s.W; a.N = s.N; a.M = s.M;
    a.kd = s.kd; a.kh = s.kh; a.kw = s.kw; a.pd = s.pd; a.ph = s.ph; a.pw = s.pw; a.dd = s.dd; a.dh = s.dh; a.dw = s.dw; a.K = s.K;
}

static void fill_igemm(IgemmArgs &a, const SameConv &s)
{
    memset(&a, 0, sizeof(a));
    copy_geom(a, s);
    a.act_bf16 = s.act_bf16;
}

// ---- dense conv forward: out = conv(x) (+ epilogue) ---------------------------------------------------------------
// wp must hold K * Cin * round_up(Cout,32) floats
// Tap splits of a launch whose partial sums meet in fp32 atomics on a zero-filled output (> 1: the caller zero-fills, and bf16 storage goes through an fp32 staging
// buffer).  Round 6: the split-operand convs (K > 1) of small volumes split their contraction over the waves of a workgroup instead (cl_conv_kw.hip: deterministic,
// no atomics) — for those this returns 1.  The deformable conv's forward keeps its own query (deform_forward_splits).
static int deform_forward_splits(const SameConv &s) { return cl_igemm_pick_splits(s.M, s.K * (s.Cin / 32), 0, s.K); }
int dense_forward_splits(const SameConv &s, int epi)
{
    const int sp = cl_igemm_pick_splits(s.M, s.K * (s.Cin / 32), epi, s.K);
    if (sp > 1 && cl_conv_kw_applies(0, s.act_bf16 ? 1 : 0, use_split(s, true), s.K, epi, round_up(s.Cout, 32), s.act_bf16 != 0, s.D > 1)) return 1;
    return sp;
}
int dense_backward_data_splits(const SameConv &s, int epi, int gout_planar)
{
    const int sp = cl_igemm_pick_splits(s.M, s.K * (round_up(s.Cout, 32) / 32), epi, s.K);
    // (gout_planar < 0: a query without the layout — bf16 storage reaches here with planar gradients only, fp32 with either)
    const int amode = gout_planar < 0 ? (s.act_bf16 ? 2 : 0) : (gout_planar ? 2 : 0);
    if (sp > 1 && cl_conv_kw_applies(amode, 0, use_split(s, false), s.K, epi, s.Cin, s.act_bf16 != 0, s.D > 1)) return 1;
    return sp;
}

// zeroed: the caller has zero-filled `out` (needed when the tap split is > 1; one batched fill per block instead of one per conv)
// ride: zero fills that go out with this launch (pointwise kernel; any other kernel gets them as a launch of their own, cl_igemm.hip)
int dense_forward(const SameConv &s, const float *x, const float *w, const float *bias, float *out, int out_planar, float *wp,
                  int epi, const float *aux, float *out2, hipStream_t st, bool zeroed, const ZeroBatch *ride, float *out2_f32)
{
    const int NP = round_up(s.Cout, 32);
    const int split = use_split(s, true);
    if (w) DLKA_TRY(launch_cl_prep_weight(w, wp, s.Cout, s.Cin, s.K, s.Cin, NP, split_mode_flag(split), st));   // w == null: wp already prepared
    IgemmArgs a;
    fill_igemm(a, s);
    a.split_bf16 = split;
    a.in = x; a.wp = wp; a.bias = bias; a.out = out; a.out2 = out2; a.aux = aux; a.epi = epi; a.out_zeroed = zeroed ? 1 : 0;
    a.Cin = s.Cin; a.CinReal = s.Cin; a.CinP = s.Cin; a.Cout = s.Cout; a.NP = NP;
    if (ride) a.zero = *ride;
    int splits = dense_forward_splits(s, epi);
    if (out_planar && cl_conv_brick3_supported(a)) splits = 1;   // (cl_conv_brick.hip writes every output itself)
    if (out2_f32) {   // only the pointwise kernel's bf16 GELU epilogue carries the fp32 side output
        if (!(s.act_bf16 && epi == 1 && s.K == 1 && splits == 1 && !split && !out_planar)) return DLKA_ERR_UNSUPPORTED;
        a.out2_f32 = out2_f32;
    }
    return launch_cl_igemm(0, out_planar ? 1 : 0, a, splits, st);
}

// ---- dense conv data gradient: gx = conv_transpose(gout) (+ epilogue) ---------------------------------------------
// wp must hold K * round_up(Cout,32) * Cin floats.  gout channels-last needs Cout % 32 == 0; planar any Cout.
// bf16 storage: `aux_f32` says the epilogue operand is fp32 all the same; `acc32` (fp32 [M][Cin], ZEROED by the caller) receives split
// partial sums and is converted into gx afterwards
int dense_backward_data(const SameConv &s, const float *gout, int gout_planar, const float *w, float *gx, float *wp, int epi,
                        const float *aux, hipStream_t st, const float *aux2, float *out2, bool zeroed, bool g_packed,
                        bool aux_f32, float *acc32, const ZeroBatch *ride)
{
    const int KP = round_up(s.Cout, 32), NP = s.Cin;
    if (!(nt_ok(NP) || NP == 192 || NP == 384) || s.Cin % 32) return DLKA_ERR_UNSUPPORTED;   // (192 / 384: the 2-D block's widths, 3 / 4 column tiles per workgroup)
    if (!gout_planar && s.Cout % 32) return DLKA_ERR_UNSUPPORTED;
    const int split = use_split(s, false);
    if (w) DLKA_TRY(launch_cl_prep_weight(w, wp, s.Cout, s.Cin, s.K, KP, NP, 1 | split_mode_flag(split), st));
    IgemmArgs a;
    fill_igemm(a, s);
    a.split_bf16 = split;
    a.pd = s.dd * (s.kd - 1) - s.pd; a.ph = s.dh * (s.kh - 1) - s.ph; a.pw = s.dw * (s.kw - 1) - s.pw;
    a.in = gout; a.wp = wp; a.bias = nullptr; a.out = gx; a.aux = aux; a.aux2 = aux2; a.out2 = out2; a.epi = epi; a.out_zeroed = zeroed ? 1 : 0;
    a.Cin = s.Cout; a.CinReal = s.Cout; a.CinP = KP; a.Cout = s.Cin; a.NP = NP;
    if (g_packed) {   // gout = pack_split2() words, KP zero-padded channel planes per batch (DeformBwdArgs::goff_cpad)
        if (!gout_planar || split != 2) return DLKA_ERR_UNSUPPORTED;
        a.a_packed = 1; a.CinReal = KP;
    }
    a.aux_f32 = aux_f32 ? 1 : 0;
    if (ride) a.zero = *ride;
    int splits = dense_backward_data_splits(s, epi, gout_planar);
    // cl_conv_brick.hip: no tap split; volumes too small for a workgroup per tile split the plane chunks instead (fp32 atomics into a zeroed buffer, like a tap split)
    const int bsplit = gout_planar ? cl_conv_brick_split(a) : 0;
    bool brick_only = false;   // the chunk split alone made this an accumulating launch: the caller's zero-fill decision (dense_backward_data_splits) does not know
    if (bsplit == 1) splits = 1;
    else if (bsplit > 1 && splits <= 1) { splits = 2; brick_only = true; }   // (only its being > 1 matters below: the zero-fill / fp32-accumulation route)
    if (s.act_bf16 && splits > 1) {
        if (!acc32) return DLKA_ERR_WORKSPACE;
        if (brick_only) DLKA_TRY(launch_zero(acc32, (size_t)s.M * s.Cin * 4, st));
        a.out = acc32; a.out_zeroed = 1;
        DLKA_TRY(launch_cl_igemm(gout_planar ? 2 : 0, 0, a, splits, st));
        return launch_cast_from_f32<bf16_t>(acc32, reinterpret_cast<bf16_t *>(gx), (long)s.M * s.Cin, st);
    }
    if (brick_only) {   // fp32 atomics into `gx`: zero it here, whatever the caller said
        DLKA_TRY(launch_zero(gx, (size_t)s.M * s.Cin * 4, st));
        a.out_zeroed = 1;
    }
    return launch_cl_igemm(gout_planar ? 2 : 0, 0, a, splits, st);
}

// (x 3/2 for K > 1: the three-term bf16 layout of the forward weights takes 48 instead of 32 floats per unit and column)
size_t dense_wp_floats(const SameConv &s) { return (size_t)s.K * round_up(s.Cin, 32) * round_up(s.Cout, 32) * (s.K > 1 ? 3 : 2) / 2; }

// ---- environment switches, read once (dlka_env_refresh() re-reads) ------------------------------------------------
static std::mutex g_fork_env_mu;
static ForkEnv g_fork_env;
static std::atomic<int> g_fork_env_loaded{0};
static void fork_env_load()
{
    std::lock_guard<std::mutex> lk(g_fork_env_mu);
    ForkEnv e;
    const char *r = getenv("DLKA_GX_FORK_MIN_ROWS");
    e.gx_rows_set = r != nullptr;
    e.gx_rows = r ? atol(r) : 0;
    const char *f = getenv("DLKA_LKA2D_FORK");
    e.lka2d_fork = !f ? 2 : f[0] == '0' ? 0 : f[0] == '1' ? 1 : 2;
    auto off = [](const char *name) { const char *v = getenv(name); return v && v[0] == '0'; };
    e.wgrad_pad = !off("DLKA_WGRAD_PAD");
    e.dwpair = !off("DLKA_DWPAIR");
    e.prep_tiled = !off("DLKA_PREP_TILED");
    g_fork_env = e;
    g_fork_env_loaded.store(1, std::memory_order_release);
}
ForkEnv fork_env()
{
    if (!g_fork_env_loaded.load(std::memory_order_acquire)) fork_env_load();
    std::lock_guard<std::mutex> lk(g_fork_env_mu);
    return g_fork_env;
}

// ---- dense conv weight gradient -----------------------------------------------------------------------------------
// padbuf (optional, dense_wgrad_pad_bytes(s) bytes): scratch for the zero-padded copy of x — selects the padded kernels (cl_wgrad.hip, round 5) where they apply
size_t dense_wgrad_pad_bytes(const SameConv &s)
{
    // (DLKA_WGRAD_PAD=0: the unpadded kernels of rounds 2 - 4.  A workspace sized with the padded copy and used without it, or the other way round, is safe — the optional
    //  carve returns null when there is no room, and null selects the unpadded kernels)
    if (!fork_env().wgrad_pad || s.K <= 1 || s.group != 1) return 0;
    const size_t n = cl_wgrad_pad_bytes(s.B, s.D, s.H, s.W, s.Cin, s.kd, s.kh, s.kw, s.dd, s.dh, s.dw, s.act_bf16);
    return n < ((size_t)1 << 31) ? align256(n) : 0;
}
int dense_backward_weight(const SameConv &s, const float *x, const float *gout, int gout_planar, float *gw, float *gb, float *part, hipStream_t st,
                          FinalizeJob *defer, int g_cpad, float *padbuf)
{
    if (s.Cin % 32) return DLKA_ERR_UNSUPPORTED;
    if (s.K != 1 && s.K > 7 * 64) return DLKA_ERR_UNSUPPORTED;
    WgradArgs a;
    memset(&a, 0, sizeof(a));
    a.g = gout; a.in = x; a.part = part;
    copy_geom(a, s);
    a.Cin = s.Cin; a.Cout = s.Cout;
    if (s.K == 1 && gout_planar) return DLKA_ERR_UNSUPPORTED;
    if (g_cpad && (!gout_planar || s.K == 1)) return DLKA_ERR_UNSUPPORTED;
    a.g_cpad = g_cpad;
    a.act_bf16 = s.act_bf16;
    a.pad = (padbuf && gout_planar && !g_cpad && dense_wgrad_pad_bytes(s)) ? padbuf : nullptr;
    return launch_cl_wgrad<float>(0, gout_planar ? 1 : 0, a, gw, gb, st, defer);
}

void fill_pw_wgrad(WgradArgs &a, const SameConv &s, const float *x, const float *gout, float *part)
{
    memset(&a, 0, sizeof(a));
    a.g = gout; a.in = x; a.part = part;
    copy_geom(a, s);
    a.Cin = s.Cin; a.Cout = s.Cout;
    a.act_bf16 = s.act_bf16;
}

// ---- depthwise ------------------------------------------------------------------------------------------------------
static void fill_dw_args(DwArgs &a, const SameConv &s, int flip)
{
    memset(&a, 0, sizeof(a));
    a.B = s.B; a.D = s.D; a.H = s.H; a.W = s.W; a.C = s.Cin;
    a.act_bf16 = s.act_bf16; a.xcd_nx = 0;
    a.kd = s.kd; a.kh = s.kh; a.dd = s.dd; a.dh = s.dh;
    if (flip) { a.pd = s.dd * (s.kd - 1) - s.pd; a.ph = s.dh * (s.kh - 1) - s.ph; a.pw = s.dw * (s.kw - 1) - s.pw; }
    else { a.pd = s.pd; a.ph = s.ph; a.pw = s.pw; }
}

int dw_forward(const SameConv &s, const float *x, const float *w, const float *bias, float *out, float *wp, int flip, hipStream_t st,
               const float *gelu_x, const float *gelu_add, float *out_lo, const DwBlk *bk)
{
    if (w) DLKA_TRY(launch_cl_dw_prep_weight(w, wp, s.Cin, s.K, flip, st));
    if (out_lo && s.act_bf16) return DLKA_ERR_UNSUPPORTED;   // (the bf16 copy rides in the fp32 kernels only)
    DwArgs a;
    fill_dw_args(a, s, flip);
    a.in = x; a.wp = wp; a.bias = bias; a.out = out; a.out_lo = out_lo; a.gelu_x = gelu_x; a.gelu_add = gelu_add;
    if (bk && bk->blk) {
        a.blk = bk->blk; a.blk_floats = bk->blk_floats; a.in_blocked = bk->in_blocked ? 1 : 0;
        if (bk->chained) *bk->chained = false;
        if (bk->chain && bk->chain_blk && cl_dwconv_lds_selected(a, s.kw, s.dw)) {
            DwArgs n;
            fill_dw_args(n, *bk->chain, flip);
            n.blk = bk->chain_blk; n.blk_floats = bk->blk_floats;
            if (cl_dwconv_lds_selected(n, bk->chain->kw, bk->chain->dw)) {
                a.out_blk = bk->chain_blk; a.out_blk_dil = bk->chain->dw;
                if (bk->chained) *bk->chained = true;
            }
        }
    }
    return launch_cl_dwconv(a, s.kw, s.dw, st);
}

// Two chained depthwise convs of a small volume in ONE launch (cl_dwpair.hip): x -> sa -> outA -> sb -> outB, prepared weights wpA / wpB (already in the wanted form: the
// flipped one for the data gradients — "same" padding is its own mirror).  DLKA_ERR_UNSUPPORTED: not that shape (or DLKA_DWPAIR=0) — the caller runs them one by one.
static int dwpair_mode()
{
    return fork_env().dwpair ? 1 : 0;
}

int dw_pair(const SameConv &sa, const SameConv &sb, const float *x, const float *wpA, const float *biasA, float *outA, float *outA_lo, const float *wpB, const float *biasB,
            float *outB, float *outB_lo, const float *gelu_x, const float *gelu_add, hipStream_t st)
{
    if (!dwpair_mode()) return DLKA_ERR_UNSUPPORTED;
    auto cubic = [](const SameConv &s) { return s.kd == s.kw && s.kh == s.kw && s.dd == s.dw && s.dh == s.dw && s.pd == s.pw && s.ph == s.pw; };
    if (!cubic(sa) || !cubic(sb) || sa.act_bf16 != sb.act_bf16 || sa.Cin != sb.Cin) return DLKA_ERR_UNSUPPORTED;
    DwPairArgs a;
    memset(&a, 0, sizeof(a));
    a.in = x; a.wpA = wpA; a.wpB = wpB; a.biasA = biasA; a.biasB = biasB; a.outA = outA; a.outB = outB; a.outA_lo = outA_lo; a.outB_lo = outB_lo;
    a.gelu_x = gelu_x; a.gelu_add = gelu_add;
    a.B = sa.B; a.D = sa.D; a.H = sa.H; a.W = sa.W; a.C = sa.Cin;
    a.kA = sa.kw; a.dA = sa.dw; a.pA = sa.pw; a.KA = sa.K;
    a.kB = sb.kw; a.dB = sb.dw; a.pB = sb.pw; a.KB = sb.K;
    a.act_bf16 = sa.act_bf16;
    return launch_cl_dwpair_small(a, st);
}

// defer != null: gwp is a zeroed [K + 1][C] staging area (row K collects the bias sums) that the caller's fused
// finalisation kernel re-lays into gw / gb
int dw_backward_weight(const SameConv &s, const float *x, const float *gout, float *gw, float *gb, float *gwp, hipStream_t st, FinalizeJob *defer)
{
    DwWgradArgs a;
    memset(&a, 0, sizeof(a));
    a.g = gout; a.in = x; a.gwp = gwp; a.gb = defer ? gwp + (size_t)s.K * s.Cin : gb;
    a.B = s.B; a.D = s.D; a.H = s.H; a.W = s.W; a.C = s.Cin;
    a.kd = s.kd; a.kh = s.kh; a.pd = s.pd; a.ph = s.ph; a.pw = s.pw; a.dd = s.dd; a.dh = s.dh;
    a.act_bf16 = s.act_bf16;
    if (defer) {
        DLKA_TRY(launch_cl_dwconv_wgrad(a, s.kw, s.dw, st, false));
        memset(defer, 0, sizeof(*defer));
        defer->part = gwp; defer->gw = gw; defer->gb = gb; defer->K = s.K; defer->Cin = s.Cin; defer->kind = 1; defer->chunks = 1;
        defer->n = (long)s.K * s.Cin + s.Cin;
        return DLKA_OK;
    }
    DLKA_TRY(launch_cl_dwconv_wgrad(a, s.kw, s.dw, st));
    return launch_cl_dw_unprep<float>(gwp, gw, s.Cin, s.K, st);
}

// ---- deformable (groups = deformable_groups = 1) ---------------------------------------------------------------------
// The deformable conv's contractions on the bf16 matrix cores (round 4): with DLKA_BF16 activations all of them (forward, Col of grad_offset / grad_input); with
// fp32 activations the two BACKWARD ones, grad_out split in two bf16 terms (fp32-equivalent to 1e-5; the forward pass keeps the exact fp32-input MFMA).  ONE
// process-wide switch, read once: DLKA_DEFORM_B16=0 keeps the fp32-input MFMA of rounds 2 - 3 everywhere (A/B runs).  It decides the layout of the prepared weights AND the kernel that reads them, so it must not change between
// a weight preparation and its use — hence cached.
bool deform_b16()
{
    static const bool on = [] { const char *e = getenv("DLKA_DEFORM_B16"); return !(e && e[0] == '0') && getenv("DLKA_EXACT_FP32") == nullptr; }();   // (DLKA_EXACT_FP32: every contraction on the fp32-input MFMA)
    return on;
}

bool deform_supported(const SameConv &s) { return s.group == 1 && s.Cin % 32 == 0 && s.Cout % 32 == 0 && nt_ok(s.Cout) && nt_ok(s.Cin); }

// Small volumes split the taps over the grid: the tap ranges' partial tiles go to `slab` (fp32 [splits][M][Cout], deform_fwd_slab_floats(s) floats, every element written)
// and are summed IN SLAB ORDER by one reduce launch — deterministic, like the reference's im2col + addmm (deform_conv_cuda.cu:95-123); rounds 1 - 5 let them meet in fp32
// atomics on a zero-filled output (the order of arrival decided the last bit, and the bf16 path needed an fp32 landing zone + a cast launch: the reduce launch replaces it).
static int deform_fwd_actual_splits(const SameConv &s) { return cl_deform_fwd_actual_splits(s.K, s.Cin, deform_forward_splits(s)); }
size_t deform_fwd_slab_floats(const SameConv &s)
{
    const int sp = deform_fwd_actual_splits(s);
    return sp > 1 ? (size_t)sp * s.M * s.Cout : 0;
}
int deform_forward(const SameConv &s, const float *x, const float *off, const float *w, const float *bias, float *out, float *wp, hipStream_t st,
                   float *slab, bool b16_cores)
{
    // DLKA_BF16: the contraction runs on the bf16 matrix cores — weights as two-term bf16 records (prep mode | 8; deform_b16() = 0 keeps the fp32-input MFMA).
    // That rounds every trilinear sample to bf16 (an ABSOLUTE error of ~2^-9 |sample| |weight| sqrt(K Cin) per output, inside the fused block's 2e-2 contract):
    // the block's choice.  b16_cores = false — the single-operator entry, "same semantics as dlka_deform_conv3d_*": bf16 STORAGE, fp32 products of the fp32
    // samples, one rounding at the store — keeps the fp32-input MFMA, as that entry's backward does (no wp16 there).
    const int b16 = (s.act_bf16 && b16_cores && deform_b16()) ? 1 : 0;
    if (w) DLKA_TRY(launch_cl_prep_weight(w, wp, s.Cout, s.Cin, s.K, s.Cin, s.Cout, b16 ? 8 : 0, st));
    IgemmArgs a;
    fill_igemm(a, s);
    a.split_bf16 = b16 ? 2 : 0;
    a.in = x; a.off = off; a.wp = wp; a.bias = bias; a.out = out; a.epi = 0; a.out_zeroed = 0;
    a.Cin = s.Cin; a.CinReal = s.Cin; a.CinP = s.Cin; a.Cout = s.Cout; a.NP = s.Cout;
    const int splits = deform_fwd_actual_splits(s);
    if (splits > 1) {
        if (!slab) return DLKA_ERR_WORKSPACE;
        a.out = slab;
        const int rc = launch_cl_deform_fwd(a, splits, st);
        if (rc == DLKA_OK) return launch_cl_slab_reduce(slab, splits, (long)s.M * s.Cout, out, s.act_bf16, st);
        if (rc != DLKA_ERR_UNSUPPORTED || s.act_bf16) return rc;
        a.out = out;   // (a width the gather kernels do not tile: the first-generation kernel, tap split with atomics on a zero fill of its own)
        return launch_cl_igemm(1, 0, a, splits, st);
    }
    const int rc = launch_cl_deform_fwd(a, 1, st);
    if (rc != DLKA_ERR_UNSUPPORTED || s.act_bf16) return rc;
    return launch_cl_igemm(1, 0, a, 1, st);
}

void fill_deform_bwd(DeformBwdArgs &a, const SameConv &s)
{
    memset(&a, 0, sizeof(a));
    copy_geom(a, s);
    a.C = s.Cin; a.Cout = s.Cout; a.CoutP = s.Cout;
    a.act_bf16 = s.act_bf16;
}

// scratch floats of the brick windows the grad_input scatter flushes (cl_deform_bwd2.hip)
size_t deform_scratch_floats(const SameConv &s)
{
    DeformBwdArgs a;
    fill_deform_bwd(a, s);
    return cl_deform_bwd2_scratch_floats(a);
}

// The stored-sample hand-over of the fp32 path keeps its samples as IEEE halves (round 6; DeformBwdArgs::samp_f16 has the reasoning and the error bound): one process-wide
// switch, read once — the grad_offset kernel that writes them and the weight-gradient kernel that reads them must agree.  DLKA_SAMP_F16=0 or DLKA_EXACT_FP32: fp32 samples.
static bool samp_f16(const SameConv &s)
{
    static const bool on = [] { const char *e = getenv("DLKA_SAMP_F16"); return !(e && e[0] == '0') && getenv("DLKA_EXACT_FP32") == nullptr; }();
    return on && !s.act_bf16;
}

int deform_backward(const SameConv &s, const float *x, const float *off, const float *w, const float *gout, float *gx, float *goff,
                    float *gw, float *gb, float *wp, float *part, float *scratch, hipStream_t st, FinalizeJob *defer, bool gx_zeroed,
                    bool goff_zeroed, int goff_cpad, float *samp, const float *wp16, bool samp_max_zeroed)
{
    // samp ([K][M][C] fp32): a grad_offset call stores the trilinear samples there, a weight-gradient call reads them instead of gathering again
    if (gx || goff) {
        if (w) DLKA_TRY(launch_cl_prep_weight(w, wp, s.Cout, s.Cin, s.K, s.Cout, s.Cin, 2, st));
        DeformBwdArgs a;
        fill_deform_bwd(a, s);
        a.in = x; a.off = off; a.g = gout; a.wp = wp; a.gx = gx; a.goff = goff; a.gx_zeroed = gx_zeroed ? 1 : 0; a.goff_zeroed = goff_zeroed ? 1 : 0; a.goff_cpad = goff_cpad;
        a.samp = goff ? samp : nullptr;
        a.samp_f16 = (a.samp && samp_f16(s)) ? 1 : 0;
        a.samp_max_zeroed = samp_max_zeroed ? 1 : 0;
        a.wp16 = deform_b16() ? wp16 : nullptr;   // (prepared by the caller: two-term bf16 records, mode 2 | 8) — both dtypes: bf16 rows as they are, fp32 rows split
        DLKA_TRY(launch_cl_deform_bwd2(a, scratch, st));
    }
    if (gw) {
        WgradArgs a;
        memset(&a, 0, sizeof(a));
        a.g = gout; a.in = x; a.off = off; a.part = part; a.samp = samp;
        a.samp_f16 = (samp && samp_f16(s)) ? 1 : 0;
        {   // DLKA_SAMP_B16MFMA=0: the half samples widened onto fp32-input MFMAs (round 6's first form); read once
            static const bool b16 = [] { const char *e = getenv("DLKA_SAMP_B16MFMA"); return !(e && e[0] == '0'); }();
            a.samp_b16mfma = (a.samp_f16 && b16) ? 1 : 0;
        }
        copy_geom(a, s);
        a.Cin = s.Cin; a.Cout = s.Cout;
        a.act_bf16 = s.act_bf16;
        DLKA_TRY(launch_cl_wgrad<float>(1, 0, a, gw, gb, st, defer));
    } else if (gb) {
        if (s.act_bf16) return DLKA_ERR_UNSUPPORTED;
        DLKA_TRY(launch_cl_colsum(gout, gb, s.M, s.Cout, st));
    }
    return DLKA_OK;
}

// conv1 + gate -> proj_2 + shortcut (bwd = 0) / their data gradients (bwd = 1) as ONE launch: C = 32 on the one-wave cl_pointwise_pair_kernel, C = 64 / 128 (256: opt-in)
// on the workgroup-tiled cl_pointwise_chain_kernel (a wave per row tile is too little parallelism there; cl_pointwise.hip).
// DLKA_PW_UNFUSED=1 keeps the two launches (A/B runs).  Returns DLKA_ERR_UNSUPPORTED when the caller has to issue the two convs itself.
int pointwise_pair(const SameConv &s, int bwd, const float *in, const float *wp1, const float *bias1, const float *wp2, const float *bias2,
                   const float *a, const float *b, float *out1, float *out1b, float *out2, hipStream_t st, const ZeroBatch *ride)
{
    const bool unfused = getenv("DLKA_PW_UNFUSED") != nullptr;   // (not cached: a parity test toggles it)
    if (unfused || s.Cin != s.Cout || s.K != 1) return DLKA_ERR_UNSUPPORTED;
    PwPairArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.in = in; pa.wp1 = wp1; pa.bias1 = bias1; pa.wp2 = wp2; pa.bias2 = bias2; pa.a = a; pa.b = b;
    pa.out1 = out1; pa.out1b = out1b; pa.out2 = out2; pa.M = s.M; pa.C = s.Cin; pa.bwd = bwd; pa.act_bf16 = s.act_bf16;
    if (ride) pa.zero = *ride;
    return s.Cin == 32 ? launch_cl_pointwise_pair(pa, st) : launch_cl_pointwise_chain(pa, st);
}

// DLKA_WGRAD_GATHER: the deformable weight gradient gathers for itself instead of streaming the samples the grad_offset kernel stored (A/B runs, the
// hand-over parity test).  Read ONCE; afterwards only dlka_lka3d_force_wgrad_gather changes it.
static std::atomic<int> g_wgrad_gather{-1};
bool wgrad_gather()
{
    int v = g_wgrad_gather.load(std::memory_order_acquire);
    if (v < 0) {
        int want = getenv("DLKA_WGRAD_GATHER") != nullptr ? 1 : 0;
        if (g_wgrad_gather.compare_exchange_strong(v, want, std::memory_order_acq_rel)) v = want;   // (lost the race: v holds the winner's value)
    }
    return v != 0;
}

void add_job(PrepBatch &pb, const void *src, float *dst, int Cout, int Cin, int K, int KP, int NP, int mode)
{
    PrepJob &j = pb.j[pb.njobs++];
    j.src = (const float *)src; j.dst = dst; j.Cout = Cout; j.Cin = Cin; j.K = K; j.KP = KP; j.NP = NP; j.mode = mode;
    if (!fork_env().prep_tiled && (mode & 7) <= 2) j.mode |= 32;   // DLKA_PREP_TILED=0: the element-per-lane re-layout (cl_igemm.hip); decided when the job is made — a test compares the two bitwise
    j.n = (mode == 3 || mode == 4) ? (long)Cin * K : (long)K * KP * NP;
    pb.total += j.n;
}

}  // namespace dlka

using namespace dlka;

extern "C" {

void dlka_env_refresh(void)
{
    fork_env_load();
}

int dlka_lka3d_force_wgrad_gather(int on)
{
    const int old = wgrad_gather() ? 1 : 0;
    g_wgrad_gather.store(on ? 1 : 0, std::memory_order_release);
    return old;
}

}  // extern "C"
