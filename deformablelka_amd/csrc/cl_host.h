// Host side of the channels-last (NDHWC / token layout) fast path, shared by the units that string the cl_*.hip kernels together: the workspace carver, the
// geometry record of a stride-1 same-size convolution, and the per-operator drivers (cl_host_ops.hip) the block drivers and the C entry points call.
// Process-wide state (cached switches) lives in cl_host_ops.hip alone and is reached through the functions declared here.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "cl_args.h"
#include "dlka_kernels.h"

namespace dlka {

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// Bump carver over a caller-provided buffer.  A buffer's layout is ONE function that carves a record of named pointers from a Carver; the forward call, the
// backward call and the size / offset queries all run that function:
//   Carver(p, n)          the real buffer: take() fails (ok() turns false) when the layout does not fit
//   Carver::measuring()   no buffer, unlimited capacity: hands out no pointers and only advances `used` — the layout's size is `used` after its carve
//   Carver::probing()     a dummy non-null base, unlimited capacity: pointers that must never be dereferenced — offset_of(field) is a field's position
struct Carver {
    uintptr_t base;
    size_t cap, used;
    bool measure;
    Carver(const void *p, size_t n) : base((uintptr_t)p), cap(n), used(0), measure(false) {}
    static Carver measuring() { Carver c(nullptr, ~(size_t)0); c.measure = true; return c; }
    static Carver probing() { return Carver((const void *)(uintptr_t)256, ~(size_t)0 >> 1); }
    void *take(size_t n)
    {
        n = align256(n);
        if (measure) { used += n; return nullptr; }
        if (!base || used + n > cap) { used = cap + 1; return nullptr; }
        void *r = (void *)(base + used);
        used += n;
        return r;
    }
    // optional area: nullptr (and the carver stays valid) when `want` is false or the buffer has no room for it
    void *take_opt(size_t n, bool want)
    {
        n = align256(n);
        if (!want) return nullptr;
        if (measure) { used += n; return nullptr; }
        if (!base || used > cap || used + n > cap) return nullptr;
        void *r = (void *)(base + used);
        used += n;
        return r;
    }
    // whether the optional area whose take_opt() returned `p` was carved (a measuring carver counts every wanted area)
    bool got(const void *p) const { return measure || p != nullptr; }
    // the next take() starts at byte `n` or later
    void skip_to(size_t n)
    {
        if (!measure && n > cap) used = cap + 1;
        else if (n > used) used = n;
    }
    size_t offset_of(const void *field) const { return (size_t)((uintptr_t)field - base); }
    bool ok() const { return used <= cap; }
};

// size of a layout: where a measuring carver stands after `carve` ran on it
template <typename Carve>
size_t carved_bytes(Carve carve)
{
    Carver m = Carver::measuring();
    carve(m);
    return m.used;
}

#define DLKA_TRY(expr)                  \
    do {                                \
        int rc_ = (expr);               \
        if (rc_ != DLKA_OK) return rc_; \
    } while (0)

// whether `s` and every member of it are set; S: a struct of nothing but pointers (dlka_lka3d_params, dlka_lka2d_grads, ...)
template <class S>
bool all_set(const S *s)
{
    static_assert(sizeof(S) % sizeof(void *) == 0, "a struct of pointers");
    const void *const *p = (const void *const *)s;
    for (size_t i = 0; p && i < sizeof(S) / sizeof(void *); ++i) if (!p[i]) return false;
    return p != nullptr;
}

// a stride-1, same-size convolution in channels-last layout
struct SameConv {
    int B, D, H, W, N, M, Cin, Cout, group;
    int kd, kh, kw, pd, ph, pw, dd, dh, dw, K;
    int act_bf16;   // 1: channels-last activation tensors are bf16 storage (DLKA_BF16 token path); planar offsets / grad_offset stay fp32
};

// environment switches, read once (dlka_env_refresh() re-reads)
struct ForkEnv {
    bool gx_rows_set;
    long gx_rows;       // DLKA_GX_FORK_MIN_ROWS
    int lka2d_fork;     // DLKA_LKA2D_FORK: 0 = one stream, 1 = the offset nets' weight gradients only, 2 (unset) = + grad_input beside grad_offset
    // A/B switches that used to be read with getenv() on every call (getenv racing with os.environ writes of other Python threads is undefined behaviour, and a
    // workspace-size query could disagree with the carve that follows it).  Tests that toggle them call dlka_env_refresh().
    bool wgrad_pad;     // DLKA_WGRAD_PAD != 0: the dense weight gradient from a zero-padded copy (cl_wgrad.hip)
    bool dwpair;        // DLKA_DWPAIR != 0: both depthwise convs of a small volume in one launch (cl_dwpair.hip)
    bool prep_tiled;    // DLKA_PREP_TILED != 0: weight preparation tile by tile through LDS (cl_igemm.hip prep_job_tile)
};
ForkEnv fork_env();   // the cached values (cl_host_ops.hip)

// The LDS-brick kernels (cl_dwconv_lds.hip) read a class-blocked fp32 copy of the input: `blk` = scratch for it (null: those kernels are never taken),
// `chain` = the depthwise conv that consumes THIS conv's output next (null: none) with `chain_blk` = scratch for ITS blocked input — when both convs take
// the LDS-brick kernel this one's epilogue writes that copy, and *chained tells the caller to pass in_blocked = true to the next call.
struct DwBlk {
    float *blk = nullptr;
    size_t blk_floats = 0;
    bool in_blocked = false;
    const SameConv *chain = nullptr;
    float *chain_blk = nullptr;
    bool *chained = nullptr;
};

// ---- per-operator drivers and their queries (cl_host_ops.hip) ----------------------------------------------------------
int make_same_conv(const dlka_conv_geom *c, SameConv &s);
bool nt_ok(int np);
bool is_depthwise(const SameConv &s);
bool dw_supported(const SameConv &s);
bool dense_fwd_supported(const SameConv &s);
int use_split(const SameConv &s, bool forward);
inline int split_mode_flag(int terms) { return terms == 3 ? 16 : (terms == 2 ? 8 : 0); }
int dense_forward_splits(const SameConv &s, int epi);
int dense_backward_data_splits(const SameConv &s, int epi, int gout_planar = -1);
int dense_forward(const SameConv &s, const float *x, const float *w, const float *bias, float *out, int out_planar, float *wp,
                  int epi, const float *aux, float *out2, hipStream_t st, bool zeroed = false, const ZeroBatch *ride = nullptr, float *out2_f32 = nullptr);
int dense_backward_data(const SameConv &s, const float *gout, int gout_planar, const float *w, float *gx, float *wp, int epi,
                        const float *aux, hipStream_t st, const float *aux2 = nullptr, float *out2 = nullptr, bool zeroed = false, bool g_packed = false,
                        bool aux_f32 = false, float *acc32 = nullptr, const ZeroBatch *ride = nullptr);
size_t dense_wp_floats(const SameConv &s);
size_t dense_wgrad_pad_bytes(const SameConv &s);
int dense_backward_weight(const SameConv &s, const float *x, const float *gout, int gout_planar, float *gw, float *gb, float *part, hipStream_t st,
                          FinalizeJob *defer = nullptr, int g_cpad = 0, float *padbuf = nullptr);
void fill_pw_wgrad(WgradArgs &a, const SameConv &s, const float *x, const float *gout, float *part);
int dw_forward(const SameConv &s, const float *x, const float *w, const float *bias, float *out, float *wp, int flip, hipStream_t st,
               const float *gelu_x = nullptr, const float *gelu_add = nullptr, float *out_lo = nullptr, const DwBlk *bk = nullptr);
int dw_pair(const SameConv &sa, const SameConv &sb, const float *x, const float *wpA, const float *biasA, float *outA, float *outA_lo, const float *wpB, const float *biasB,
            float *outB, float *outB_lo, const float *gelu_x, const float *gelu_add, hipStream_t st);
int dw_backward_weight(const SameConv &s, const float *x, const float *gout, float *gw, float *gb, float *gwp, hipStream_t st, FinalizeJob *defer = nullptr);
bool deform_b16();
bool deform_supported(const SameConv &s);
size_t deform_fwd_slab_floats(const SameConv &s);
int deform_forward(const SameConv &s, const float *x, const float *off, const float *w, const float *bias, float *out, float *wp, hipStream_t st,
                   float *slab = nullptr, bool b16_cores = true);
void fill_deform_bwd(DeformBwdArgs &a, const SameConv &s);
size_t deform_scratch_floats(const SameConv &s);
int deform_backward(const SameConv &s, const float *x, const float *off, const float *w, const float *gout, float *gx, float *goff,
                    float *gw, float *gb, float *wp, float *part, float *scratch, hipStream_t st, FinalizeJob *defer = nullptr, bool gx_zeroed = false,
                    bool goff_zeroed = false, int goff_cpad = 0, float *samp = nullptr, const float *wp16 = nullptr, bool samp_max_zeroed = false);
int pointwise_pair(const SameConv &s, int bwd, const float *in, const float *wp1, const float *bias1, const float *wp2, const float *bias2,
                   const float *a, const float *b, float *out1, float *out1b, float *out2, hipStream_t st, const ZeroBatch *ride = nullptr);
bool wgrad_gather();
void add_job(PrepBatch &pb, const void *src, float *dst, int Cout, int Cin, int K, int KP, int NP, int mode);
}  // namespace dlka
