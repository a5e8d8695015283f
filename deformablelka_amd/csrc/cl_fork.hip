// The per-device pool of fork contexts behind ForkLease (cl_fork.h: the CONTRACT), the fork decision of the 3-D backward pass and the diagnostics export.
#include <atomic>
#include <mutex>

#include "cl_fork.h"

namespace dlka {

constexpr int FORK_MAX_DEV = 64;
static std::atomic<long> g_fork_created_dev[FORK_MAX_DEV], g_fork_leases_dev[FORK_MAX_DEV];   // diagnostics (dlka_fork_stats)

#if !defined(HIPEMU)
static std::mutex g_fork_mu;
static ForkCtx *g_fork_free[FORK_MAX_DEV];
static std::atomic<int> g_fork_failed{0};      // creation failed once: no forks in this process

static ForkCtx *fork_ctx_create(int dev)
{
    ForkCtx *c = new ForkCtx();
    memset(c, 0, sizeof(*c));
    c->dev = dev;
    bool ok = hipStreamCreateWithFlags(&c->s, hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithFlags(&c->s2, hipStreamNonBlocking) == hipSuccess;
    hipEvent_t *evs[] = {&c->fork, &c->join, &c->fork2, &c->join2};
    for (hipEvent_t *e : evs) ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    if (!ok) {   // (no stale error for the next launch check to find; the handles created so far are released)
        (void)hipGetLastError();
        if (c->s) (void)hipStreamDestroy(c->s);
        if (c->s2) (void)hipStreamDestroy(c->s2);
        for (hipEvent_t *e : evs) if (*e) (void)hipEventDestroy(*e);
        (void)hipGetLastError();
        delete c;
        return nullptr;
    }
    g_fork_created_dev[dev].fetch_add(1, std::memory_order_relaxed);
    return c;
}

ForkLease::ForkLease(hipStream_t st, bool want) : st_(st)
{
    if (!want || g_fork_failed.load(std::memory_order_acquire)) return;
    int dev = -1, sdev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= FORK_MAX_DEV) { (void)hipGetLastError(); return; }
    if (st && hipStreamGetDevice(st, &sdev) == hipSuccess && sdev != dev) return;   // a foreign stream: the launches themselves will say so; no fork
    (void)hipGetLastError();
    if (!capture_of(st, &cap_)) return;
    {
        std::lock_guard<std::mutex> lk(g_fork_mu);
        ForkCtx **pp = &g_fork_free[dev];
        while (*pp) {
            ForkCtx *c = *pp;
            bool usable = true;
            if (c->cap_id) {   // pulled into a capture by an earlier call: is that capture over by now, or is it this very capture?
                unsigned long long i1 = 0, i2 = 0;
                const bool q = capture_of(c->s, &i1) && capture_of(c->s2, &i2);
                if (q && !i1 && !i2) c->cap_id = 0;
                else usable = q && cap_ != 0 && cap_ == c->cap_id;
            }
            if (usable) { *pp = c->next; c->next = nullptr; c_ = c; break; }
            pp = &c->next;
        }
    }
    if (!c_ && cap_ == 0) {   // none free for this device: create one — never inside a capture
        c_ = fork_ctx_create(dev);
        if (!c_) g_fork_failed.store(1, std::memory_order_release);
    }
    if (c_) g_fork_leases_dev[dev].fetch_add(1, std::memory_order_relaxed);
}

ForkLease::~ForkLease()
{
    if (!c_) return;
    // an early return between a fork and its join: join now, whatever the streams hold (best effort; the call is failing anyway)
    if (open1_) (void)join(1);
    if (open2_) (void)join(2);
    (void)hipGetLastError();
    if (cap_) c_->cap_id = cap_;
    std::lock_guard<std::mutex> lk(g_fork_mu);
    c_->next = g_fork_free[c_->dev];
    g_fork_free[c_->dev] = c_;
}
#endif

bool gx_fork_wanted(long rows, int phase)
{
#if defined(HIPEMU)
    (void)rows; (void)phase;
    return false;   // (no streams on the CPU test backend)
#else
    const ForkEnv e = fork_env();
    if (!e.gx_rows_set) return phase == 1;
    return rows >= e.gx_rows;
#endif
}

}  // namespace dlka

using namespace dlka;

extern "C" {

// ---- fork contexts: diagnostics ------------------------------------------------------------------------------------------
int dlka_fork_stats(int device, int64_t *contexts, int64_t *leases)
{
    if (device < 0 || device >= FORK_MAX_DEV) return DLKA_ERR_SHAPE;
    if (contexts) *contexts = g_fork_created_dev[device].load(std::memory_order_relaxed);
    if (leases) *leases = g_fork_leases_dev[device].load(std::memory_order_relaxed);
    return DLKA_OK;
}

}  // extern "C"
