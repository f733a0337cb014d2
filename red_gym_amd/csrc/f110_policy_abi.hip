// f110_policy_abi.hip -- part of the C ABI (include/f110_hip.h) over the gfx950 kernels; see f110_common.h for the units.
#include "f110_common.h"
#include "f110_policyhead.h"
#include "f110_qhead.h"
#include "f110_adam.h"
#include "f110_adam_clip.h"
#include "f110_sacloss.h"
#include "f110_temperature.h"

// ---------------------------------------------------------------- policy head: fc_mean, fc_log_std and the sampling tail
extern "C" int f110_policyhead_validate(const f110_policyhead_config *cfg) { return policyhead_check(cfg, "f110_policyhead_validate"); }

extern "C" int64_t f110_policyhead_workspace(const f110_policyhead_config *cfg, int64_t n)
{
    if (n < 1 || n > PH_MAX_ROWS || f110_policyhead_validate(cfg) != F110_OK) return 0;
    return policyhead_workspace_bytes(*cfg, n);
}

extern "C" int f110_policyhead_forward(const f110_policyhead_config *cfg, const float *h, int64_t n, const float *w_mean, const float *b_mean,
                                       const float *w_log_std, const float *b_log_std, const float *eps, float *pre, void *action, void *log_prob,
                                       void *stream)
{
    const char *who = "f110_policyhead_forward";
    if (int rc = f110_policyhead_validate(cfg)) return rc;
    if (n < 0 || n > PH_MAX_ROWS) return fail(F110_E_INVALID, "%s: n=%lld rows (0..%lld)", who, (long long)n, (long long)PH_MAX_ROWS);
    if (n == 0) return F110_OK;
    if (!h || !w_mean || !w_log_std || !pre || !action) return fail(F110_E_INVALID, "%s: null pointer", who);
    if ((eps == nullptr) != (log_prob == nullptr)) return fail(F110_E_INVALID, "%s: log_prob must be NULL exactly when eps is NULL", who);
    if (int rc = check_device_pointers(who, (hipStream_t)stream, {{"h", h}, {"w_mean", w_mean}, {"w_log_std", w_log_std}, {"pre", pre}, {"action", action}})) return rc;
    PolicyheadForwardPlan p = policyhead_forward_plan(*cfg, n);
    PolicyheadArgs &a = p.a;
    a.h = h; a.w_mean = w_mean; a.b_mean = b_mean; a.w_log_std = w_log_std; a.b_log_std = b_log_std; a.eps = eps;
    a.pre = pre; a.action = action; a.log_prob = log_prob;
#define POLICYHEAD_FWD(T, F64) F110_LAUNCH((policyhead_forward_kernel<T, F64>), p.l, (hipStream_t)stream, a)
    switch (p.l.inst) { case 2 * 1: POLICYHEAD_FWD(1, false); break; case 2 * 1 + 1: POLICYHEAD_FWD(1, true); break;
                        case 2 * 2: POLICYHEAD_FWD(2, false); break; default: POLICYHEAD_FWD(2, true); break; }
#undef POLICYHEAD_FWD
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_policyhead_backward(const f110_policyhead_config *cfg, const float *h, int64_t n, const float *w_mean, const float *w_log_std,
                                        const float *pre, const float *eps, const void *grad_action, const void *grad_log_prob, const float *grad_pre,
                                        float *grad_h, float *grad_w_mean, float *grad_b_mean, float *grad_w_log_std, float *grad_b_log_std, float *workspace,
                                        void *stream)
{
    const char *who = "f110_policyhead_backward";
    if (int rc = f110_policyhead_validate(cfg)) return rc;
    if (n < 0 || n > PH_MAX_ROWS) return fail(F110_E_INVALID, "%s: n=%lld rows (0..%lld)", who, (long long)n, (long long)PH_MAX_ROWS);
    if (n == 0) return F110_OK;
    if (!h || !w_mean || !w_log_std || !pre || !grad_action || !workspace) return fail(F110_E_INVALID, "%s: null pointer", who);
    if (!eps && grad_log_prob) return fail(F110_E_INVALID, "%s: grad_log_prob without eps (no log_prob was produced)", who);
    if ((uintptr_t)workspace % 16) return fail(F110_E_INVALID, "%s: the workspace must be 16-byte aligned", who);
    if (int rc = check_device_pointers(who, (hipStream_t)stream, {{"h", h}, {"w_mean", w_mean}, {"w_log_std", w_log_std}, {"pre", pre},
                                                                    {"grad_action", grad_action}, {"workspace", workspace}})) return rc;
    PolicyheadBackwardPlan p = policyhead_backward_plan(*cfg, n);
    PolicyheadArgs &a = p.a;
    a.h = h; a.w_mean = w_mean; a.w_log_std = w_log_std; a.eps = eps; a.pre = const_cast<float *>(pre);
    a.grad_action = grad_action; a.grad_log_prob = grad_log_prob; a.grad_pre = grad_pre;
    a.gpre = workspace + p.gpre_at; a.partial = workspace + p.partial_at;
    a.grad_h = grad_h; a.grad_w_mean = grad_w_mean; a.grad_b_mean = grad_b_mean; a.grad_w_log_std = grad_w_log_std; a.grad_b_log_std = grad_b_log_std;
    hipStream_t s = (hipStream_t)stream;
    if (p.gpre.inst) F110_LAUNCH(policyhead_gpre_kernel<true>, p.gpre, s, a);
    else F110_LAUNCH(policyhead_gpre_kernel<false>, p.gpre, s, a);
    HIP_TRY(hipGetLastError());
    if (grad_h) {
        F110_LAUNCH(policyhead_gradh_kernel, p.gradh, s, a);
        HIP_TRY(hipGetLastError());
    }
    if (grad_w_mean || grad_b_mean || grad_w_log_std || grad_b_log_std) {
        F110_LAUNCH(policyhead_gradw_kernel, p.gradw, s, a);
        HIP_TRY(hipGetLastError());
        F110_LAUNCH(policyhead_reduce_kernel, p.reduce, s, a);
        HIP_TRY(hipGetLastError());
    }
    return F110_OK;
}

// ---------------------------------------------------------------- critic head: the twin Q tail and the TD target
extern "C" int f110_qhead_validate(const f110_qhead_config *cfg) { return qhead_check(cfg, "f110_qhead_validate"); }

extern "C" int64_t f110_qhead_workspace(const f110_qhead_config *cfg, int64_t n)
{
    if (n < 1 || n > QH_MAX_ROWS || f110_qhead_validate(cfg) != F110_OK) return 0;
    return qhead_workspace_bytes(*cfg, n);
}

// what both entry points ask of the critics' arrays; the pointers that must be device memory are appended to `ptrs`
static int qhead_critics(const char *who, const f110_qhead_config *cfg, const f110_qhead_critics *p, QheadArgs &a, std::vector<DevicePtr> &ptrs)
{
    static const char *names[3][QH_MAX_C] = {{"pre[0]", "pre[1]"}, {"w_act[0]", "w_act[1]"}, {"w2[0]", "w2[1]"}};
    for (int c = 0; c < cfg->critics; c++) {
        if (!p->pre[c] || !p->w_act[c] || !p->w2[c]) return fail(F110_E_INVALID, "%s: null pre, w_act or w2 of critic %d", who, c);
        a.pre[c] = p->pre[c]; a.w_act[c] = p->w_act[c]; a.b1[c] = p->b1[c]; a.w2[c] = p->w2[c]; a.b2[c] = p->b2[c];
        ptrs.push_back({names[0][c], p->pre[c]}); ptrs.push_back({names[1][c], p->w_act[c]}); ptrs.push_back({names[2][c], p->w2[c]});
    }
    return F110_OK;
}

// the forward entry points; alpha_dev: where the target's alpha is read on the device, NULL: `alpha`; by_row: the target's discount is
// read per row from discount_dev [n], else `gamma`
static int qhead_forward(const char *who, const f110_qhead_config *cfg, const f110_qhead_critics *p, const void *action, int64_t n,
                         const double *reward, const uint8_t *done, const void *next_log_prob, double gamma, double alpha, bool by_pointer,
                         const double *alpha_dev, float *q, float *qmin, float *target, void *stream, bool by_row = false,
                         const double *discount_dev = nullptr)
{
    if (int rc = f110_qhead_validate(cfg)) return rc;
    if (n < 0 || n > QH_MAX_ROWS) return fail(F110_E_INVALID, "%s: n=%lld rows (0..%lld)", who, (long long)n, (long long)QH_MAX_ROWS);
    if (n == 0) return F110_OK;
    if (!p || !action || !q) return fail(F110_E_INVALID, "%s: null pointer", who);
    if (target && (!reward || !done || !next_log_prob)) return fail(F110_E_INVALID, "%s: a target needs reward, done and next_log_prob", who);
    if (target && (!std::isfinite(gamma) || !std::isfinite(alpha))) return fail(F110_E_INVALID, "%s: gamma or alpha is not finite", who);
    if (target && by_pointer && !alpha_dev) return fail(F110_E_INVALID, "%s: null alpha", who);
    if (target && by_row && !discount_dev) return fail(F110_E_INVALID, "%s: null discount", who);
    QheadForwardPlan plan = qhead_forward_plan(*cfg, n);
    QheadArgs &a = plan.a;
    std::vector<DevicePtr> ptrs = {{"action", action}, {"q", q}};
    if (int rc = qhead_critics(who, cfg, p, a, ptrs)) return rc;
    if (target) { ptrs.push_back({"reward", reward}); ptrs.push_back({"done", done}); ptrs.push_back({"next_log_prob", next_log_prob}); ptrs.push_back({"target", target}); }
    if (target && by_pointer) ptrs.push_back({"alpha", alpha_dev});
    if (target && by_row) ptrs.push_back({"discount", discount_dev});
    if (int rc = check_device_pointers(who, (hipStream_t)stream, ptrs)) return rc;
    a.action = action; a.q = q; a.qmin = qmin; a.target = target;
    if (target) { a.reward = reward; a.done = done; a.nlp = next_log_prob; a.gamma = gamma; a.alpha = alpha; a.alpha_dev = by_pointer ? alpha_dev : nullptr; a.discount_dev = by_row ? discount_dev : nullptr; }
    F110_LAUNCH(qhead_forward_kernel, plan.l, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_qhead_forward(const f110_qhead_config *cfg, const f110_qhead_critics *p, const void *action, int64_t n, const double *reward,
                                  const uint8_t *done, const void *next_log_prob, double gamma, double alpha, float *q, float *qmin, float *target,
                                  void *stream)
{
    return qhead_forward("f110_qhead_forward", cfg, p, action, n, reward, done, next_log_prob, gamma, alpha, false, nullptr, q, qmin, target, stream);
}

extern "C" int f110_qhead_forward_alpha_dev(const f110_qhead_config *cfg, const f110_qhead_critics *p, const void *action, int64_t n,
                                            const double *reward, const uint8_t *done, const void *next_log_prob, double gamma, const double *alpha,
                                            float *q, float *qmin, float *target, void *stream)
{
    return qhead_forward("f110_qhead_forward_alpha_dev", cfg, p, action, n, reward, done, next_log_prob, gamma, 0.0, true, alpha, q, qmin, target, stream);
}

extern "C" int f110_qhead_forward_rows(const f110_qhead_config *cfg, const f110_qhead_critics *p, const void *action, int64_t n, const double *reward,
                                       const uint8_t *done, const void *next_log_prob, const double *discount, double alpha, const double *alpha_dev,
                                       float *q, float *qmin, float *target, void *stream)
{
    // (gamma is unused; 0.0 passes the finiteness check.  A non-null alpha_dev wins, and `alpha` is then not looked at)
    const bool by_pointer = alpha_dev != nullptr;
    return qhead_forward("f110_qhead_forward_rows", cfg, p, action, n, reward, done, next_log_prob, 0.0, by_pointer ? 0.0 : alpha, by_pointer, alpha_dev, q,
                         qmin, target, stream, true, discount);
}

extern "C" int f110_qhead_backward(const f110_qhead_config *cfg, const f110_qhead_critics *p, const void *action, int64_t n, const float *q,
                                   const float *grad_q, const float *grad_qmin, const f110_qhead_grads *g, void *grad_action, float *workspace,
                                   void *stream)
{
    const char *who = "f110_qhead_backward";
    if (int rc = f110_qhead_validate(cfg)) return rc;
    if (n < 0 || n > QH_MAX_ROWS) return fail(F110_E_INVALID, "%s: n=%lld rows (0..%lld)", who, (long long)n, (long long)QH_MAX_ROWS);
    if (n == 0) return F110_OK;
    if (!p || !action || !q || !g) return fail(F110_E_INVALID, "%s: null pointer", who);
    if ((uintptr_t)workspace % 16) return fail(F110_E_INVALID, "%s: the workspace must be 16-byte aligned", who);
    QheadBackwardPlan plan = qhead_backward_plan(*cfg, n);
    QheadArgs &a = plan.a;
    std::vector<DevicePtr> ptrs = {{"action", action}, {"q", q}};
    if (int rc = qhead_critics(who, cfg, p, a, ptrs)) return rc;
    bool rows = grad_action != nullptr, params = false;
    for (int c = 0; c < a.C; c++) {
        a.grad_pre[c] = g->grad_pre[c]; a.grad_w_act[c] = g->grad_w_act[c]; a.grad_b1[c] = g->grad_b1[c]; a.grad_w2[c] = g->grad_w2[c]; a.grad_b2[c] = g->grad_b2[c];
        rows = rows || a.grad_pre[c];
        params = params || a.grad_w_act[c] || a.grad_b1[c] || a.grad_w2[c] || a.grad_b2[c];
    }
    if (params && !workspace) return fail(F110_E_INVALID, "%s: parameter gradients need the workspace", who);
    if (params) ptrs.push_back({"workspace", workspace});
    if (int rc = check_device_pointers(who, (hipStream_t)stream, ptrs)) return rc;
    a.action = action; a.q_in = q; a.grad_q = grad_q; a.grad_qmin = grad_qmin; a.grad_action = grad_action;
    a.partial = workspace + plan.partial_at;
    hipStream_t s = (hipStream_t)stream;
    if (rows) {
        if (plan.rows.inst == 16) F110_LAUNCH(qhead_rows_kernel<16>, plan.rows, s, a);
        else F110_LAUNCH(qhead_rows_kernel<32>, plan.rows, s, a);
        HIP_TRY(hipGetLastError());
    }
    if (params) {
        if (plan.gradw.inst == 16) F110_LAUNCH(qhead_gradw_kernel<16>, plan.gradw, s, a);
        else F110_LAUNCH(qhead_gradw_kernel<32>, plan.gradw, s, a);
        HIP_TRY(hipGetLastError());
        F110_LAUNCH(qhead_reduce_kernel, plan.reduce, s, a);
        HIP_TRY(hipGetLastError());
    }
    return F110_OK;
}

// ---------------------------------------------------------------- parameter update: Adam and the soft update of the targets
static int adam_scalar_checks(const char *who, const f110_adam_config *cfg, bool target)
{
    if (!cfg) return fail(F110_E_INVALID, "%s: null config", who);
    if (!(cfg->beta1 >= 0.0 && cfg->beta1 < 1.0)) return fail(F110_E_INVALID, "%s: beta1 %g (0 <= beta1 < 1)", who, cfg->beta1);
    if (!(cfg->beta2 >= 0.0 && cfg->beta2 < 1.0)) return fail(F110_E_INVALID, "%s: beta2 %g (0 <= beta2 < 1)", who, cfg->beta2);
    if (!std::isfinite(cfg->eps) || !(cfg->eps > 0.0)) return fail(F110_E_INVALID, "%s: eps %g (finite and > 0)", who, cfg->eps);
    if (target && (!std::isfinite(cfg->tau) || cfg->tau < 0.0 || cfg->tau > 1.0)) return fail(F110_E_INVALID, "%s: tau %g (0 <= tau <= 1)", who, cfg->tau);
    return F110_OK;
}

extern "C" int f110_adam_validate(const f110_adam_config *cfg)
{
    return adam_scalar_checks("f110_adam_validate", cfg, cfg && cfg->with_target);
}

extern "C" int64_t f110_adam_state_bytes(void) { return (int64_t)sizeof(f110_adam_state); }

// the checks on the table and the kernel's copy of it -> chunks of the launch in *grid
static int adam_table(const char *who, const f110_adam_tensor *table, int n_tensors, bool adam, bool target, AdamTable &tab, uint32_t *grid,
                      std::vector<DevicePtr> &ptrs)
{
    if (n_tensors < 0 || n_tensors > AD_MAX_T) return fail(F110_E_INVALID, "%s: n_tensors %d (0..%d a call)", who, n_tensors, AD_MAX_T);
    if (n_tensors > 0 && !table) return fail(F110_E_INVALID, "%s: null table", who);
    memset(&tab, 0, sizeof(tab));
    tab.n_tensors = n_tensors;
    uint32_t chunks = 0;
    for (int i = 0; i < n_tensors; i++) {
        const f110_adam_tensor &t = table[i];
        if (t.n < 0 || t.n > ((int64_t)1 << 31)) return fail(F110_E_INVALID, "%s: tensor %d: n %lld (0..2^31)", who, i, (long long)t.n);
        if (t.n > 0) {
            if (!t.p) return fail(F110_E_INVALID, "%s: tensor %d: null p", who, i);
            if (adam && !t.m) return fail(F110_E_INVALID, "%s: tensor %d: null m", who, i);
            if (adam && !t.v) return fail(F110_E_INVALID, "%s: tensor %d: null v", who, i);
            if (adam && !t.g) return fail(F110_E_INVALID, "%s: tensor %d: null g", who, i);
            if (target && !t.target) return fail(F110_E_INVALID, "%s: tensor %d: null target", who, i);
            if (target && t.target == t.p) return fail(F110_E_INVALID, "%s: tensor %d: target == p", who, i);
            uintptr_t bits = (uintptr_t)t.p;
            if (adam) bits |= (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v;
            if (target) bits |= (uintptr_t)t.target;
            if (bits % 4) return fail(F110_E_INVALID, "%s: tensor %d: a pointer is not 4-byte aligned", who, i);
            AdamEntry &e = tab.t[i];
            e.p = t.p; e.n = (uint32_t)t.n; e.vec = bits % 16 == 0;
            if (adam) { e.g = t.g; e.m = t.m; e.v = t.v; }
            if (target) e.target = t.target;
            chunks += (uint32_t)((t.n + AD_CHUNK - 1) / AD_CHUNK);
            ptrs.push_back({"p", t.p});
            if (target) ptrs.push_back({"target", t.target});
        }
        tab.chunk_end[i] = chunks;      // (at most 64 * 2^19)
    }
    *grid = chunks;
    return F110_OK;
}

// f110_adam_step (clip NULL: the launches it always made) and f110_adam_step_clipped
static int adam_step(const char *who, const f110_adam_config *cfg, const f110_adam_tensor *table, int32_t n_tensors, f110_adam_state *state,
                     const f110_adam_clip_state *clip, bool clipped, double lr, void *stream)
{
    if (int rc = adam_scalar_checks(who, cfg, cfg && cfg->with_target)) return rc;
    if (!state) return fail(F110_E_INVALID, "%s: null state", who);
    if ((uintptr_t)state % 8) return fail(F110_E_INVALID, "%s: the state is not 8-byte aligned", who);
    if (clipped && !clip) return fail(F110_E_INVALID, "%s: null clip", who);
    if (clipped && (uintptr_t)clip % 8) return fail(F110_E_INVALID, "%s: clip is not 8-byte aligned", who);
    if (!std::isfinite(lr)) return fail(F110_E_INVALID, "%s: lr is not finite", who);
    const bool target = cfg->with_target != 0;
    AdamTable tab;
    uint32_t grid = 0;
    std::vector<DevicePtr> ptrs = {{"state", state}};
    if (clipped) ptrs.push_back({"clip", clip});
    if (int rc = adam_table(who, table, n_tensors, true, target, tab, &grid, ptrs)) return rc;
    if (int rc = check_device_pointers(who, (hipStream_t)stream, ptrs)) return rc;
    tab.c1 = (float)(1.0 - cfg->beta1); tab.c2 = (float)(1.0 - cfg->beta2); tab.b2 = (float)cfg->beta2; tab.eps = (float)cfg->eps;
    tab.tau = target ? (float)cfg->tau : 0.0f;
    hipStream_t s = (hipStream_t)stream;
    if (cfg->advance) {
        if (clipped) hipLaunchKernelGGL(adam_advance_clip_kernel, dim3(1), dim3(64), 0, s, state, clip, cfg->beta1, cfg->beta2, lr);
        else hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, s, state, cfg->beta1, cfg->beta2, lr);
        HIP_TRY(hipGetLastError());
    }
    if (grid == 0) return F110_OK;
    if (clipped) {
        if (target) hipLaunchKernelGGL((adam_clipped_kernel<true>), dim3(grid), dim3(AD_THREADS), 0, s, tab, (const AdamState *)state, clip);
        else hipLaunchKernelGGL((adam_clipped_kernel<false>), dim3(grid), dim3(AD_THREADS), 0, s, tab, (const AdamState *)state, clip);
    } else {
        if (target) hipLaunchKernelGGL((adam_kernel<true, true>), dim3(grid), dim3(AD_THREADS), 0, s, tab, (const AdamState *)state);
        else hipLaunchKernelGGL((adam_kernel<true, false>), dim3(grid), dim3(AD_THREADS), 0, s, tab, (const AdamState *)state);
    }
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_adam_step(const f110_adam_config *cfg, const f110_adam_tensor *table, int32_t n_tensors, f110_adam_state *state, double lr,
                              void *stream)
{
    return adam_step("f110_adam_step", cfg, table, n_tensors, state, nullptr, false, lr, stream);
}

extern "C" int f110_soft_update(const f110_adam_tensor *table, int32_t n_tensors, double tau, void *stream)
{
    const char *who = "f110_soft_update";
    if (!std::isfinite(tau) || tau < 0.0 || tau > 1.0) return fail(F110_E_INVALID, "%s: tau %g (0 <= tau <= 1)", who, tau);
    AdamTable tab;
    uint32_t grid = 0;
    std::vector<DevicePtr> ptrs;
    if (int rc = adam_table(who, table, n_tensors, false, true, tab, &grid, ptrs)) return rc;
    if (grid == 0) return F110_OK;
    if (int rc = check_device_pointers(who, (hipStream_t)stream, ptrs)) return rc;
    tab.tau = (float)tau;
    hipLaunchKernelGGL((adam_kernel<false, true>), dim3(grid), dim3(AD_THREADS), 0, (hipStream_t)stream, tab, (const AdamState *)nullptr);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

// ---------------------------------------------------------------- gradient clipping: the global norm, the coefficient, the guard
extern "C" int64_t f110_adam_clip_state_bytes(void) { return (int64_t)sizeof(f110_adam_clip_state); }

extern "C" int f110_adam_gradnorm(const f110_adam_tensor *table, int32_t n_tensors, int64_t chunk_base, double *partials, int64_t partials_len,
                                  void *stream)
{
    const char *who = "f110_adam_gradnorm";
    if (int rc = adam_gradnorm_check(who, chunk_base, partials, partials_len, -1)) return rc;
    if (n_tensors < 0 || n_tensors > AD_MAX_T) return fail(F110_E_INVALID, "%s: n_tensors %d (0..%d a call)", who, n_tensors, AD_MAX_T);
    if (n_tensors > 0 && !table) return fail(F110_E_INVALID, "%s: null table", who);
    AdamTable tab;
    memset(&tab, 0, sizeof(tab));
    tab.n_tensors = n_tensors;
    int64_t chunks = 0;
    for (int i = 0; i < n_tensors; i++) {
        const f110_adam_tensor &t = table[i];
        if (t.n < 0 || t.n > ((int64_t)1 << 31)) return fail(F110_E_INVALID, "%s: tensor %d: n %lld (0..2^31)", who, i, (long long)t.n);
        if (t.n > 0) {
            if (!t.g) return fail(F110_E_INVALID, "%s: tensor %d: null g", who, i);
            if ((uintptr_t)t.g % 4) return fail(F110_E_INVALID, "%s: tensor %d: g is not 4-byte aligned", who, i);
            tab.t[i].g = t.g; tab.t[i].n = (uint32_t)t.n; tab.t[i].vec = (uintptr_t)t.g % 16 == 0;
            chunks += adam_chunks(t.n);
        }
        tab.chunk_end[i] = (uint32_t)chunks;
    }
    if (int rc = adam_gradnorm_check(who, chunk_base, partials, partials_len, chunks)) return rc;
    if (int rc = check_device_pointers(who, (hipStream_t)stream, {{"partials", partials}})) return rc;
    if (chunks == 0) return F110_OK;
    hipLaunchKernelGGL(adam_gradnorm_kernel, dim3((uint32_t)chunks), dim3(AC_THREADS), 0, (hipStream_t)stream, tab, partials + chunk_base);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_adam_clip(const double *partials, int64_t n_chunks, double max_norm, f110_adam_clip_state *clip, void *stream)
{
    const char *who = "f110_adam_clip";
    if (int rc = adam_clip_check(who, partials, n_chunks, max_norm, clip)) return rc;
    if (int rc = check_device_pointers(who, (hipStream_t)stream, {{"partials", partials}, {"clip", clip}})) return rc;
    hipLaunchKernelGGL(adam_clip_kernel, dim3(1), dim3(AC_THREADS), 0, (hipStream_t)stream, partials, (long long)n_chunks, max_norm, clip);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_adam_step_clipped(const f110_adam_config *cfg, const f110_adam_tensor *table, int32_t n_tensors, f110_adam_state *state,
                                      const f110_adam_clip_state *clip, double lr, void *stream)
{
    return adam_step("f110_adam_step_clipped", cfg, table, n_tensors, state, clip, true, lr, stream);
}

// ---------------------------------------------------------------- the two losses of a SAC update and their gradients
static int sacloss_rows(const char *who, int64_t n)
{
    if (n < 1 || n > SL_MAX_ROWS) return fail(F110_E_INVALID, "%s: n=%lld rows (1..%lld)", who, (long long)n, (long long)SL_MAX_ROWS);
    return F110_OK;
}

extern "C" int f110_sac_critic_loss(const float *q1, const float *q2, const float *tv, int64_t n, float *loss, float *grad_q1, float *grad_q2,
                                    void *stream)
{
    const char *who = "f110_sac_critic_loss";
    if (int rc = sacloss_rows(who, n)) return rc;
    if (!q1 || !q2 || !tv || !loss) return fail(F110_E_INVALID, "%s: null pointer", who);
    std::vector<DevicePtr> ptrs = {{"q1", q1}, {"q2", q2}, {"tv", tv}, {"loss", loss}};
    if (grad_q1) ptrs.push_back({"grad_q1", grad_q1});
    if (grad_q2) ptrs.push_back({"grad_q2", grad_q2});
    if (int rc = check_device_pointers(who, (hipStream_t)stream, ptrs)) return rc;
    SaclossPlan p = sacloss_plan(n, false, false, 0.0);
    p.a.q1 = q1; p.a.q2 = q2; p.a.tv = tv; p.a.loss = loss; p.a.grad_q1 = grad_q1; p.a.grad_q2 = grad_q2;
    F110_LAUNCH(sac_critic_loss_kernel, p.l, (hipStream_t)stream, p.a);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_sac_critic_loss_weighted(const float *q1, const float *q2, const float *tv, const float *w, int64_t n, float *loss,
                                             float *grad_q1, float *grad_q2, float *td_out, void *stream)
{
    const char *who = "f110_sac_critic_loss_weighted";
    if (int rc = sacloss_rows(who, n)) return rc;
    if (!q1 || !q2 || !tv || !loss) return fail(F110_E_INVALID, "%s: null pointer", who);
    if (!w) return fail(F110_E_INVALID, "%s: null w", who);
    std::vector<DevicePtr> ptrs = {{"q1", q1}, {"q2", q2}, {"tv", tv}, {"w", w}, {"loss", loss}};
    if (grad_q1) ptrs.push_back({"grad_q1", grad_q1});
    if (grad_q2) ptrs.push_back({"grad_q2", grad_q2});
    if (td_out) ptrs.push_back({"td_out", td_out});
    if (int rc = check_device_pointers(who, (hipStream_t)stream, ptrs)) return rc;
    SaclossPlan p = sacloss_plan(n, false, false, 0.0);
    p.a.q1 = q1; p.a.q2 = q2; p.a.tv = tv; p.a.w = w; p.a.loss = loss; p.a.grad_q1 = grad_q1; p.a.grad_q2 = grad_q2; p.a.td_out = td_out;
    F110_LAUNCH(sac_critic_loss_weighted_kernel, p.l, (hipStream_t)stream, p.a);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

// both actor-loss entry points; alpha_dev: where alpha is read on the device, NULL: `alpha`
static int sac_actor_loss(const char *who, const void *logp, int32_t logp_fp64, const float *qn, double alpha, bool by_pointer, const double *alpha_dev,
                          int64_t n, float *loss, void *grad_logp, float *grad_qn, void *stream)
{
    if (int rc = sacloss_rows(who, n)) return rc;
    if (!logp || !qn || !loss) return fail(F110_E_INVALID, "%s: null pointer", who);
    if (by_pointer && !alpha_dev) return fail(F110_E_INVALID, "%s: null alpha", who);
    if (!std::isfinite(alpha)) return fail(F110_E_INVALID, "%s: alpha is not finite", who);
    if ((uintptr_t)logp % (logp_fp64 ? 8 : 4) || (uintptr_t)grad_logp % (logp_fp64 ? 8 : 4))
        return fail(F110_E_INVALID, "%s: logp or grad_logp is not aligned to its type", who);
    std::vector<DevicePtr> ptrs = {{"logp", logp}, {"qn", qn}, {"loss", loss}};
    if (grad_logp) ptrs.push_back({"grad_logp", grad_logp});
    if (grad_qn) ptrs.push_back({"grad_qn", grad_qn});
    if (by_pointer) ptrs.push_back({"alpha", alpha_dev});
    if (int rc = check_device_pointers(who, (hipStream_t)stream, ptrs)) return rc;
    SaclossPlan p = sacloss_plan(n, true, logp_fp64 != 0, alpha);
    p.a.logp = logp; p.a.qn = qn; p.a.loss = loss; p.a.grad_logp = grad_logp; p.a.grad_qn = grad_qn;
    p.a.alpha_dev = by_pointer ? alpha_dev : nullptr;
    if (p.l.inst == 2) F110_LAUNCH(sac_actor_loss_kernel<true>, p.l, (hipStream_t)stream, p.a);
    else F110_LAUNCH(sac_actor_loss_kernel<false>, p.l, (hipStream_t)stream, p.a);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_sac_actor_loss(const void *logp, int32_t logp_fp64, const float *qn, double alpha, int64_t n, float *loss, void *grad_logp,
                                   float *grad_qn, void *stream)
{
    return sac_actor_loss("f110_sac_actor_loss", logp, logp_fp64, qn, alpha, false, nullptr, n, loss, grad_logp, grad_qn, stream);
}

extern "C" int f110_sac_actor_loss_alpha_dev(const void *logp, int32_t logp_fp64, const float *qn, const double *alpha, int64_t n, float *loss,
                                             void *grad_logp, float *grad_qn, void *stream)
{
    return sac_actor_loss("f110_sac_actor_loss_alpha_dev", logp, logp_fp64, qn, 0.0, true, alpha, n, loss, grad_logp, grad_qn, stream);
}

// ---------------------------------------------------------------- the entropy temperature learnt on the device
extern "C" int f110_temperature_validate(const f110_temperature_config *cfg) { return temperature_check(cfg, "f110_temperature_validate"); }

extern "C" int64_t f110_temperature_state_bytes(void) { return (int64_t)sizeof(f110_temperature_state); }

extern "C" int f110_temperature_step(const f110_temperature_config *cfg, const void *logp, int32_t logp_fp64, int64_t n,
                                     f110_temperature_state *state, double lr, void *stream)
{
    const char *who = "f110_temperature_step";
    if (int rc = temperature_step_check(who, cfg, logp, logp_fp64, n, state, lr)) return rc;
    if (int rc = check_device_pointers(who, (hipStream_t)stream, {{"logp", logp}, {"state", state}})) return rc;
    TemperaturePlan p = temperature_plan(*cfg, n, logp_fp64 != 0, lr);
    p.a.logp = logp; p.a.state = state;
    if (p.l.inst) F110_LAUNCH(temperature_step_kernel<true>, p.l, (hipStream_t)stream, p.a);
    else F110_LAUNCH(temperature_step_kernel<false>, p.l, (hipStream_t)stream, p.a);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}
