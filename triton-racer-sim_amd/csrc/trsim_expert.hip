// trsim_expert.hip — the scripted expert of libtrsim.so (include/trsim_spec.h, "scripted expert"): the device-resident stand-in for the reference's human
// driver (components/controller.py:24).  One kernel, trs_expert_kernel, evaluates the rule for one env per thread; trs_expert_act hands out the pure
// labels, trs_step_expert closes the loop in the shape of trs_step_pilot (trsim_pilot.hip) and can capture (frame, label row) records into device memory.
// The host side of the decisions (config checks, track_yaw, which ticks are captured) is trsim_expert.hpp.  The handle is reached as in the control and
// JPEG units: trsim_env.hpp and the accessors of trsim_internal.hpp.
// The kernel is bound by its launch: about 60 B per env, no LDS, no atomics, 256-thread workgroups on a grid of ceil(n / 256).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/trsim.h"
#include "../../include/trsim_spec.h"
#include "trsim_env.hpp"
#include "trsim_expert.hpp"
#include "trsim_internal.hpp"

namespace {

using trsim::kExpertRowFloats;

struct ExpertParams {
    // the env's state (the truth): views into the handle's slab
    const int32_t* seg_idx; const float *yaw, *cte, *speed; const uint8_t* done;
    const float *track_yaw, *profile /* nullptr: +inf */, *target;
    float* w;                           // the disturbance state per env; nullptr: the pure rule (trs_expert_act)
    float *out_steer, *out_thr, *out_brk;   // the applied controls (the labels when w == nullptr)
    float* rows;                        // float[n][8] of the slot a captured tick goes to, or nullptr
    int n, np, look, env_id_base;
    float k_cte, k_head, thr_hi, thr_lo, brake_over, brake_val, alpha, sigma;
    unsigned long long seed;
    uint32_t k;                         // the driver's tick counter
};

__device__ __forceinline__ float clamp1(float v) { return fminf(fmaxf(v, -1.0f), 1.0f); }

__global__ __launch_bounds__(256) void trs_expert_kernel(const ExpertParams p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n) return;
    const int seg = p.seg_idx[i];
    const float yaw = p.yaw[i], cte = p.cte[i], speed = p.speed[i];
    int j = (seg + p.look) % p.np;
    if (j < 0) j += p.np;                                    // (an index is never negative; the table is never read out of bounds either way)
    float herr = yaw - p.track_yaw[j];
    if (herr > TRS_PI) herr -= TRS_TWO_PI;
    if (herr < -TRS_PI) herr += TRS_TWO_PI;
    const float a = p.k_cte * cte, b = p.k_head * herr;
    const float steer = clamp1(-(a + b));
    float v_ref = p.target[i];
    if (p.profile) v_ref = fminf(v_ref, p.profile[j]);
    const float thr = speed < v_ref ? p.thr_hi : p.thr_lo;
    const float brk = speed > v_ref * p.brake_over ? p.brake_val : 0.0f;
    float applied = steer;
    if (p.w) {
        const unsigned long long gid = (unsigned long long)(unsigned)(p.env_id_base + i);
        unsigned long long z = p.seed + ((gid << 32) | (unsigned long long)p.k) * 0x9E3779B97F4A7C15ull;
        z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
        z ^= z >> 27; z *= 0x94D049BB133111EBull;
        z ^= z >> 31;
        const float u = (float)(z >> 40) * 5.9604644775390625e-08f;        // 2^-24
        const float raw = u * 2.0f - 1.0f;
        float w = p.w[i];
        const float d = p.sigma * raw - w;
        w = w + p.alpha * d;
        p.w[i] = w;
        applied = clamp1(steer + w);
    }
    p.out_steer[i] = applied; p.out_thr[i] = thr; p.out_brk[i] = brk;
    if (p.rows) {
        const float segment = (float)((double)seg / (double)p.np * 10.0);
        float* r = p.rows + (size_t)i * kExpertRowFloats;   // (dword stores: the caller's array need not be aligned beyond a float)
        r[trsim::kExpertRowSteer] = steer; r[trsim::kExpertRowThr] = thr; r[trsim::kExpertRowBrk] = brk; r[trsim::kExpertRowApplied] = applied;
        r[trsim::kExpertRowSpeed] = speed; r[trsim::kExpertRowCte] = cte; r[trsim::kExpertRowSegment] = segment;
        r[trsim::kExpertRowDone] = p.done[i] ? 1.0f : 0.0f;
    }
}

// what trs_set_expert keeps per handle (behind trs_internal_expert_slot); its buffers are the project's owning type
struct ExpertCtx {
    trs_expert_config cfg{};
    trsim::DevBuf<float> track_yaw, profile, target, w;
    bool has_profile = false;
    int n = 0, n_points = 0;
    uint32_t k = 0;                     // ticks driven since trs_set_expert
};

ExpertParams params_of(const trs_env* e, const ExpertCtx* c, int n)
{
    ExpertParams p{};
    p.seg_idx = e->pp.seg_idx; p.yaw = e->pp.yaw; p.cte = e->pp.cte; p.speed = e->pp.speed; p.done = e->pp.done;
    p.track_yaw = c->track_yaw.get(); p.profile = c->has_profile ? c->profile.get() : nullptr; p.target = c->target.get();
    p.n = n; p.np = c->n_points; p.look = c->cfg.look; p.env_id_base = e->cfg.env_id_base;
    p.k_cte = c->cfg.k_cte; p.k_head = c->cfg.k_head; p.thr_hi = c->cfg.thr_hi; p.thr_lo = c->cfg.thr_lo;
    p.brake_over = c->cfg.brake_over; p.brake_val = c->cfg.brake_val; p.alpha = c->cfg.alpha; p.sigma = c->cfg.sigma;
    p.seed = c->cfg.seed; p.k = c->k;
    return p;
}

int launch_expert(const trs_env* e, const ExpertParams& p)
{
    hipLaunchKernelGGL(trs_expert_kernel, dim3((p.n + 255) / 256), dim3(256), 0, e->sP, p);
    HIPCHK(hipGetLastError());
    return TRS_OK;
}

ExpertCtx* ctx_of(trs_env* e) { return static_cast<ExpertCtx*>(*trs_internal_expert_slot(e)); }

}  // namespace

void trs_expert_free(void* ctx) { delete static_cast<ExpertCtx*>(ctx); }

TRS_EXPORT void trs_default_expert_config(trs_expert_config* cfg)
{
    if (cfg) trsim::expert_defaults(cfg);
}

TRS_EXPORT int trs_set_expert(trs_env* e, const trs_expert_config* cfg, const float* h_target, const float* h_profile)
{
    if (!e) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    if (cfg && !e->track_loaded) return trs_internal_fail(TRS_ERR_STATE, "no track loaded");
    const int np = e->pp.np;
    if (cfg) {
        if (const char* why = trsim::expert_config_error(cfg, np)) return trs_internal_fail(TRS_ERR_ARG, why);
    }
    HIPCHK(hipSetDevice(e->device));
    { int rc = trsim::sync_handle(e); if (rc) return rc; }   // the buffers that go may still be read by queued launches
    void** slot = trs_internal_expert_slot(e);
    if (!cfg) {
        trs_expert_free(*slot);
        *slot = nullptr;
        return TRS_OK;
    }
    // build the new driver beside the old one: a failure below leaves the handle as it was
    ExpertCtx* c = new ExpertCtx;
    struct Guard { ExpertCtx* c; ~Guard() { delete c; } } guard{c};
    c->cfg = *cfg; c->n = e->n; c->n_points = np; c->has_profile = h_profile != nullptr;
    std::vector<float> ty((size_t)np), tg((size_t)e->n);
    trsim::build_track_yaw(e->tab.tangent.data(), np, ty.data());
    for (int i = 0; i < e->n; ++i) tg[(size_t)i] = h_target ? h_target[i] : cfg->target_speed;
    HIPCHK(c->track_yaw.alloc((size_t)np * 4));
    HIPCHK(c->target.alloc((size_t)e->n * 4));
    HIPCHK(c->w.alloc((size_t)e->n * 4));
    if (h_profile) HIPCHK(c->profile.alloc((size_t)np * 4));
    HIPCHK(hipMemcpy(c->track_yaw.get(), ty.data(), (size_t)np * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->target.get(), tg.data(), (size_t)e->n * 4, hipMemcpyHostToDevice));
    if (h_profile) HIPCHK(hipMemcpy(c->profile.get(), h_profile, (size_t)np * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(c->w.get(), 0, (size_t)e->n * 4));
    trs_internal_count(e, 0, (size_t)np * 4 * (h_profile ? 2 : 1) + (size_t)e->n * 4);
    trs_expert_free(*slot);
    *slot = c;
    guard.c = nullptr;
    return TRS_OK;
}

TRS_EXPORT int trs_expert_act(trs_env* e, float* d_steer, float* d_thr, float* d_brk, int n)
{
    if (!e) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    ExpertCtx* c = ctx_of(e);
    if (!c) return trs_internal_fail(TRS_ERR_STATE, "no expert set (trs_set_expert)");
    if (!d_steer || !d_thr || !d_brk || n < 0 || n > e->n) return trs_internal_fail(TRS_ERR_ARG, "null output or n out of range (n <= n_envs)");
    HIPCHK(hipSetDevice(e->device));
    if (n == 0) return TRS_OK;
    { int rq = trsim::quiesce_handle(e); if (rq) return rq; }   // the kernel goes onto the handle's stream and reads the state behind the posted steps
    ExpertParams p = params_of(e, c, n);
    p.out_steer = d_steer; p.out_thr = d_thr; p.out_brk = d_brk;
    int rc = launch_expert(e, p);
    if (!rc) trsim::resident_note_launch(e);                 // resident mode selected: this kernel has no completion flag, trs_sync waits for the stream
    return rc;
}

TRS_EXPORT int trs_step_expert(trs_env* e, int n_steps, const trs_expert_capture* cap, int* n_captured)
{
    if (!e) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    ExpertCtx* c = ctx_of(e);
    if (!c) return trs_internal_fail(TRS_ERR_STATE, "no expert set (trs_set_expert)");
    if (n_steps < 1) return trs_internal_fail(TRS_ERR_ARG, "n_steps < 1");
    if (const char* why = trsim::expert_capture_error(cap, e->cfg.render != 0)) return trs_internal_fail(TRS_ERR_ARG, why);
    HIPCHK(hipSetDevice(e->device));
    trsim::CapturePlan plan = trsim::CapturePlan::of(cap);
    if (n_captured) *n_captured = 0;
    const size_t row_stride = (size_t)e->n * kExpertRowFloats;
    for (int t = 0; t < n_steps; ++t) {
        TrsEnvView v;
        if (!trs_internal_view(e, &v)) return trs_internal_fail(TRS_ERR_DEVICE, "the handle's stream could not be taken over from the resident worker");
        const uint8_t* frame = cap && cap->d_frames_or_null ? v.latest_frame : nullptr;      // the rendered truth of the state the label is computed on
        const int slot = cap ? plan.slot_for(c->k, !cap->d_frames_or_null || frame != nullptr) : -1;
        ExpertParams p = params_of(e, c, e->n);
        p.w = c->w.get();
        p.out_steer = v.ctl_steer; p.out_thr = v.ctl_thr; p.out_brk = v.ctl_brk;
        p.rows = slot >= 0 ? cap->d_rows + (size_t)slot * row_stride : nullptr;
        int rc = launch_expert(e, p);
        if (rc) return rc;
        c->k += 1;                                           // the disturbance state has moved: the counter moves with it
        if (slot >= 0 && frame)                              // in front of the step: the buffer is recycled two steps on
            HIPCHK(hipMemcpyAsync(cap->d_frames_or_null + (size_t)slot * e->img_bytes, frame, e->img_bytes, hipMemcpyDeviceToDevice, v.stream));
        if (n_captured) *n_captured = plan.used;
        rc = trs_internal_step_launch(e, v.ctl_steer, v.ctl_thr, v.ctl_brk);
        if (rc) return rc;
    }
    return TRS_OK;
}
