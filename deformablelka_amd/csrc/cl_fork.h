// Fork / join of independent kernels of ONE library call onto library-internal streams: the leased context (ForkCtx), its RAII lease (ForkLease) and the
// fork decision of the 3-D backward pass.  The pool and the counters — the state — are in cl_fork.hip, with the functions that touch them.
#pragma once
#include "cl_host.h"

namespace dlka {

// ---- fork / join inside the backward passes -----------------------------------------------------------------------------
// Two places let independent kernels of ONE call run beside each other on library-internal streams (events fork from and join back into the caller's stream; under
// hipGraph capture the pattern becomes a fork / join in the graph):
//   * grad_input of the 3-D deformable conv beside grad_offset (stream `s`; the stack engine's data-chain pass, see gx_fork_wanted),
//   * the 2-D block's offset-net weight gradients (`s`) and its depthwise deformable convs' grad_input (`s2`) beside the data chain (lka2d_cl_backward).
// Why the pairs pay (profiles/r06_notes.md, `r7d`, `r7h`, `r7i`): at the 32^3 stage grad_input beside grad_offset gains 35 us per block (the LDS-window scatter kernel runs
// two workgroups per CU at 128 registers, the gather kernel three waves per SIMD with little LDS — they fill each other's holes); forking EVERY block measured best in the
// whole step on three boxes (fp32 10.616 / 10.597 / 10.518 ms for never / wide stage only / always).
//
// CONTRACT.  The streams and events a call forks onto are a ForkCtx LEASED for the duration of that call from a per-DEVICE pool:
//   * per device: a context is created on the device the caller's stream belongs to (== the current device, or the call does not fork at all), so a call under
//     nn.DataParallel on device k never touches a handle of device 0 (2D/trainer_MaxViT_deform_LKA.py:107-108 wraps the model so);
//   * per caller: two host threads (each on its own stream) inside the library at the same time hold DIFFERENT contexts — no event is shared between concurrent calls;
//     a context returns to the pool when its call returns (everything it forked has been joined into the caller's stream by then, so stream order carries the
//     dependency on to whoever leases it next);
//   * capture: contexts are never CREATED inside a stream capture (a capturing call finds one in the pool or keeps everything on the caller's stream); a context whose
//     streams were pulled into a capture is handed only to calls of that same capture until the capture has ended;
//   * errors: a lease that has forked and is destroyed without its join (early return on a failed launch) still joins its streams into the caller's, so neither
//     an eager caller nor a capture is left with an unjoined stream.
#if !defined(HIPEMU)
struct ForkCtx {
    int dev;
    hipStream_t s, s2;
    hipEvent_t fork, join, fork2, join2;
    unsigned long long cap_id;        // != 0: last used inside the stream capture with this id
    ForkCtx *next;
};

// RAII lease of one ForkCtx for one library call on the caller's stream `st`.  ok() == false: the call keeps everything on `st`.
class ForkLease {
    ForkCtx *c_ = nullptr;
    hipStream_t st_;
    unsigned long long cap_ = 0;
    bool open1_ = false, open2_ = false;

    static bool capture_of(hipStream_t s, unsigned long long *id)
    {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        unsigned long long i = 0;
        if (hipStreamGetCaptureInfo(s, &cs, &i) != hipSuccess) { (void)hipGetLastError(); *id = 0; return false; }
        *id = cs == hipStreamCaptureStatusActive ? (i ? i : ~0ull) : 0;
        return cs == hipStreamCaptureStatusNone || cs == hipStreamCaptureStatusActive;
    }

public:
    ForkLease(hipStream_t st, bool want);
    ForkLease(const ForkLease &) = delete;
    ForkLease &operator=(const ForkLease &) = delete;
    ~ForkLease();
    bool ok() const { return c_ != nullptr; }
    // which: 1 = stream s (events fork / join), 2 = stream s2 (fork2 / join2).  fork() may be repeated before one join() (the stream then also sees the later work).
    hipStream_t stream(int which) const { return !c_ ? st_ : which == 2 ? c_->s2 : c_->s; }
    int fork(int which)   // the internal stream may use what the caller's stream has produced so far
    {
        if (!c_) return DLKA_OK;
        hipEvent_t e = which == 2 ? c_->fork2 : c_->fork;
        if (hipEventRecord(e, st_) != hipSuccess || hipStreamWaitEvent(stream(which), e, 0) != hipSuccess) return DLKA_ERR_LAUNCH;
        (which == 2 ? open2_ : open1_) = true;
        return DLKA_OK;
    }
    int join(int which)   // the caller's stream waits for everything issued on the internal stream so far
    {
        if (!c_) return DLKA_OK;
        bool &open = which == 2 ? open2_ : open1_;
        if (!open) return DLKA_OK;
        open = false;
        hipEvent_t e = which == 2 ? c_->join2 : c_->join;
        if (hipEventRecord(e, stream(which)) != hipSuccess || hipStreamWaitEvent(st_, e, 0) != hipSuccess) return DLKA_ERR_LAUNCH;
        return DLKA_OK;
    }
};

#else   // HIPEMU: no streams on the CPU test backend — every lease is empty and the call stays on the caller's stream
class ForkLease {
    hipStream_t st_;
public:
    ForkLease(hipStream_t st, bool) : st_(st) {}
    bool ok() const { return false; }
    hipStream_t stream(int) const { return st_; }
    int fork(int) { return DLKA_OK; }
    int join(int) { return DLKA_OK; }
};
#endif

// Environment switches of the fork decisions, read ONCE (dlka_env_refresh() re-reads: tests and the A/B scripts toggle them in-process).
// (phase 0 = the one-call backward of the nn.Module path: there the fork measured SLOWER — wrapper-block stack 100.5 against 102.5 volumes/s, full net 68.8 against 69.8 — so by
//  default only the stack engine's data-chain pass, phase 1, forks; DLKA_GX_FORK_MIN_ROWS = row count from which a call forks (a huge value = never), when set, rules both)
bool gx_fork_wanted(long rows, int phase);

}  // namespace dlka
