// C-ABI entry points of the UNETR++ efficient paired attention (cl_epa.hip): float32, hidden_size / heads in {8, 16, 32, 64}, proj_size in {32, 64}.
// Anything else returns DLKA_ERR_UNSUPPORTED (the size queries 0) and the module runs the same forward operator by operator.
#include "cl_host.h"

using namespace dlka;

namespace {

bool epa_ok(int C, int heads, int P, int dtype)
{
    if (dtype != DLKA_F32 || heads <= 0 || C <= 0 || C % heads) return false;
    const int D = C / heads;
    return (D == 8 || D == 16 || D == 32 || D == 64) && (P == 32 || P == 64);
}

// the saved statistics of one forward call: nrm [B][5][C], then ghat, a_soft, a_mask, each [B][heads][D][D]
struct EpaSaved {
    float *nrm, *ghat, *a_soft, *a_mask;
};
EpaSaved epa_saved(void *p, int B, int C, int heads)
{
    const size_t dd = (size_t)B * C * (C / heads);
    float *f = (float *)p;
    return EpaSaved{f, f + (size_t)B * 5 * C, f + (size_t)B * 5 * C + dd, f + (size_t)B * 5 * C + 2 * dd};
}

struct EpaWs {
    float *gpart, *tpart, *dgh, *proj;
};
EpaWs epa_carve(Carver &cv, int B, int N, int C, int heads, int P, int backward)
{
    EpaWs w{};
    const int D = C / heads;
    w.gpart = (float *)cv.take(epa_gram_part_floats(B, N, heads, D) * 4);
    if (backward) {
        w.tpart = (float *)cv.take(epa_token_part_floats(B, N, heads, D, P) * 4);
        w.dgh = (float *)cv.take((size_t)B * C * D * 4);
        w.proj = (float *)cv.take((size_t)B * 2 * C * 4);
    }
    return w;
}

bool epa_sizes_ok(int B, int N, int C, int P) { return B > 0 && N > 0 && (double)B * N * 4 * C < 2147483648.0 && (double)B * 4 * N * P < 2147483648.0; }

}  // namespace

extern "C" {

int dlka_epa_supported(int C, int heads, int P, int dtype) { return epa_ok(C, heads, P, dtype) ? 1 : 0; }

size_t dlka_epa_saved_bytes(int B, int C, int heads)
{
    if (B <= 0 || heads <= 0 || C <= 0 || C % heads) return 0;
    return (size_t)B * C * (5 + 3 * (size_t)(C / heads)) * 4;
}

size_t dlka_epa_workspace_bytes(int B, int N, int C, int heads, int P, int backward)
{
    if (!epa_ok(C, heads, P, DLKA_F32) || !epa_sizes_ok(B, N, C, P)) return 0;
    Carver cv = Carver::measuring();
    epa_carve(cv, B, N, C, heads, P, backward);
    return cv.used;
}

int dlka_epa_attention_forward(const void *qkvv, const void *kp, const void *vp, const void *temperature, const void *temperature2, const void *m1,
                               const void *m2, float m2_scale, void *x_sa, void *x_ca, void *saved, void *workspace, size_t workspace_bytes, int B, int N,
                               int C, int heads, int P, int dtype, void *stream)
{
    if (!qkvv || !kp || !vp || !temperature || !temperature2 || !x_sa || !x_ca || !saved) return DLKA_ERR_NULL;
    if (dtype != DLKA_F32) return DLKA_ERR_DTYPE;
    if (B <= 0 || N <= 0 || C <= 0 || heads <= 0 || P <= 0) return DLKA_ERR_SHAPE;
    if (!epa_ok(C, heads, P, dtype) || !epa_sizes_ok(B, N, C, P)) return DLKA_ERR_UNSUPPORTED;
    Carver cv(workspace, workspace_bytes);
    const EpaWs w = epa_carve(cv, B, N, C, heads, P, 0);
    if (!cv.ok()) return DLKA_ERR_WORKSPACE;
    const EpaSaved s = epa_saved(saved, B, C, heads);
    hipStream_t st = (hipStream_t)stream;
    const float *q = (const float *)qkvv;
    const int D = C / heads;
    DLKA_TRY(launch_cl_epa_gram(q, (long)N * 4 * C, 4 * C, 0, q, (long)N * 4 * C, 4 * C, C, w.gpart, B, N, heads, D, true, st));
    DLKA_TRY(launch_cl_epa_finish(w.gpart, (const float *)temperature, (const float *)temperature2, (const float *)m1, s.nrm, s.ghat, s.a_soft, s.a_mask, B, N, C,
                                  heads, st));
    return launch_cl_epa_apply(q, (const float *)kp, (const float *)vp, m1 ? s.a_mask : s.a_soft, s.nrm, (const unsigned char *)m2, m2_scale, (float *)x_sa,
                               (float *)x_ca, B, N, C, heads, P, st);
}

int dlka_epa_attention_backward(const void *qkvv, const void *kp, const void *vp, const void *temperature, const void *temperature2, const void *m1,
                                const void *m2, float m2_scale, const void *saved, const void *g_x_sa, const void *g_x_ca, void *g_qkvv, void *g_kp,
                                void *g_vp, void *g_temperature_bh, void *g_temperature2_bh, void *workspace, size_t workspace_bytes, int B, int N, int C,
                                int heads, int P, int dtype, void *stream)
{
    if (!qkvv || !kp || !vp || !temperature || !temperature2 || !saved || !g_x_sa || !g_x_ca || !g_qkvv || !g_kp || !g_vp || !g_temperature_bh ||
        !g_temperature2_bh)
        return DLKA_ERR_NULL;
    if (dtype != DLKA_F32) return DLKA_ERR_DTYPE;
    if (B <= 0 || N <= 0 || C <= 0 || heads <= 0 || P <= 0) return DLKA_ERR_SHAPE;
    if (!epa_ok(C, heads, P, dtype) || !epa_sizes_ok(B, N, C, P)) return DLKA_ERR_UNSUPPORTED;
    Carver cv(workspace, workspace_bytes);
    const EpaWs w = epa_carve(cv, B, N, C, heads, P, 1);
    if (!cv.ok()) return DLKA_ERR_WORKSPACE;
    const EpaSaved s = epa_saved(const_cast<void *>(saved), B, C, heads);
    hipStream_t st = (hipStream_t)stream;
    const float *q = (const float *)qkvv;
    const float *am = m1 ? s.a_mask : s.a_soft;
    const int D = C / heads;
    DLKA_TRY(launch_cl_epa_bwd_tokens(q, (const float *)kp, (const float *)vp, s.nrm, (const float *)temperature2, (const unsigned char *)m2, m2_scale,
                                      (const float *)g_x_sa, (float *)g_qkvv, w.tpart, B, N, C, heads, P, st));
    DLKA_TRY(launch_cl_epa_gram((const float *)g_x_ca, (long)N * C, C, 0, q, (long)N * 4 * C, 4 * C, 2 * C, w.gpart, B, N, heads, D, false, st));
    DLKA_TRY(launch_cl_epa_bwd_finish(w.gpart, w.tpart, (const float *)kp, (const float *)temperature, (const float *)temperature2, (const float *)m1, s.a_soft,
                                      s.ghat, s.nrm, (float *)g_kp, (float *)g_vp, (float *)g_temperature_bh, (float *)g_temperature2_bh, w.dgh, w.proj, B, N, C,
                                      heads, P, st));
    return launch_cl_epa_bwd_apply(q, am, w.dgh, s.nrm, w.proj, (const float *)g_x_ca, (float *)g_qkvv, B, N, C, heads, st);
}

}  // extern "C"
