// trsim_expert.hip — the scripted expert of libtrsim.so (include/trsim_spec.h, "scripted expert"): the device-resident stand-in for the reference's human
// driver (components/controller.py:24).  The rule is one __device__ function, expert_label, evaluated for one env per thread by two kernels:
// trs_expert_kernel (trs_expert_act hands out the pure labels, trs_step_expert closes the loop) and trs_dagger_kernel (trs_step_dagger, "pilot in the loop
// with the expert's labels": the pilot has acted, the expert labels the truth, a keyed gate decides per car who holds the wheel).  Both loops can capture
// (frame, label row) records into device memory.
// A closed loop here is its argument checks and an ops object (ExpertOps, DaggerOps: what observes, what labels) handed to trsim::closed_loop of
// trsim_loop.hpp, which owns the order of a tick, the capture plan and the counter; trs_step_pilot (trsim_pilot.hip) runs through the same loop.
// The other host-side decisions (config checks, track_yaw, the gate) are trsim_expert.hpp.  The handle is reached as in the control and JPEG units:
// trsim_env.hpp and the accessors of trsim_internal.hpp.
// The kernels are bound by their launch: about 60 B (dagger: about 100 B) per env, no LDS, no atomics, 256-thread workgroups on a grid of ceil(n / 256).
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

using trsim::kDaggerStatFloats;
using trsim::kExpertRowFloats;

// what the rule reads: the env's state (the truth, views into the handle's slab), the driver's tables and its constants
struct ExpertRule {
    const int32_t* seg_idx; const float *yaw, *cte, *speed; const uint8_t* done;
    const float *track_yaw, *profile /* nullptr: +inf */, *target;
    int np, look;
    float k_cte, k_head, thr_hi, thr_lo, brake_over, brake_val;
};

struct ExpertParams {
    ExpertRule rule;
    float* w;                           // the disturbance state per env; nullptr: the pure rule (trs_expert_act)
    float *out_steer, *out_thr, *out_brk;   // the applied controls (the labels when w == nullptr)
    float* rows;                        // float[n][8] of the slot a captured tick goes to, or nullptr
    int n, env_id_base;
    float alpha, sigma;
    unsigned long long seed;
    uint32_t k;                         // the driver's tick counter
};

struct DaggerParams {
    ExpertRule rule;
    float *ctl_steer, *ctl_thr, *ctl_brk;   // in: the pilot's controls of this tick; out: the applied controls
    float* rows;                        // float[n][8] of the slot a captured tick goes to, or nullptr
    float* stats;                       // float[n][6]
    int n, env_id_base, expert_speed;
    float beta;
    unsigned long long seed;
    uint32_t block;                     // k / hold of the driver's tick counter
};

__device__ __forceinline__ float clamp1(float v) { return fminf(fmaxf(v, -1.0f), 1.0f); }

// the label of env i and the state it was computed on
struct ExpertLabel { float steer, thr, brk, speed, cte; int seg; };

__device__ __forceinline__ ExpertLabel expert_label(const ExpertRule& p, int i)
{
    ExpertLabel l;
    l.seg = p.seg_idx[i];
    const float yaw = p.yaw[i];
    l.cte = p.cte[i]; l.speed = p.speed[i];
    int j = (l.seg + p.look) % p.np;
    if (j < 0) j += p.np;                                    // (an index is never negative; the table is never read out of bounds either way)
    float herr = yaw - p.track_yaw[j];
    if (herr > TRS_PI) herr -= TRS_TWO_PI;
    if (herr < -TRS_PI) herr += TRS_TWO_PI;
    const float a = p.k_cte * l.cte, b = p.k_head * herr;
    l.steer = clamp1(-(a + b));
    float v_ref = p.target[i];
    if (p.profile) v_ref = fminf(v_ref, p.profile[j]);
    l.thr = l.speed < v_ref ? p.thr_hi : p.thr_lo;
    l.brk = l.speed > v_ref * p.brake_over ? p.brake_val : 0.0f;
    return l;
}

// a record row of env i: the label, the steering the car was given and the state the label was computed on
__device__ __forceinline__ void write_row(float* rows, const ExpertRule& p, int i, const ExpertLabel& l, float applied)
{
    const float segment = (float)((double)l.seg / (double)p.np * 10.0);
    float* r = rows + (size_t)i * kExpertRowFloats;         // (dword stores: the caller's array need not be aligned beyond a float)
    r[trsim::kExpertRowSteer] = l.steer; r[trsim::kExpertRowThr] = l.thr; r[trsim::kExpertRowBrk] = l.brk; r[trsim::kExpertRowApplied] = applied;
    r[trsim::kExpertRowSpeed] = l.speed; r[trsim::kExpertRowCte] = l.cte; r[trsim::kExpertRowSegment] = segment;
    r[trsim::kExpertRowDone] = p.done[i] ? 1.0f : 0.0f;
}

__global__ __launch_bounds__(256) void trs_expert_kernel(const ExpertParams p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n) return;
    const ExpertLabel l = expert_label(p.rule, i);
    float applied = l.steer;
    if (p.w) {
        const float u = trsim::unit24(trsim::splitmix64(p.seed, trsim::env_key((uint32_t)(p.env_id_base + i), p.k)));
        const float raw = u * 2.0f - 1.0f;
        float w = p.w[i];
        const float d = p.sigma * raw - w;
        w = w + p.alpha * d;
        p.w[i] = w;
        applied = clamp1(l.steer + w);
    }
    p.out_steer[i] = applied; p.out_thr[i] = l.thr; p.out_brk[i] = l.brk;
    if (p.rows) write_row(p.rows, p.rule, i, l, applied);
}

// One tick of "pilot in the loop with the expert's labels" between the pilot's tail and the env step: the control arrays hold the pilot's controls and leave
// with the applied ones.  block, seed, beta and expert_speed are kernel arguments: uniform over the wave, they stay in scalar registers.
__global__ __launch_bounds__(256) void trs_dagger_kernel(const DaggerParams p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n) return;
    const ExpertLabel l = expert_label(p.rule, i);
    const float ps = p.ctl_steer[i];
    const bool expert = trsim::dagger_gate(p.seed, (uint32_t)(p.env_id_base + i), p.block, p.beta);
    const float applied = expert ? l.steer : ps;
    p.ctl_steer[i] = applied;
    if (p.expert_speed || expert) { p.ctl_thr[i] = l.thr; p.ctl_brk[i] = l.brk; }   // else: the pilot's throttle and brake stay where they are
    if (p.rows) write_row(p.rows, p.rule, i, l, applied);
    const float acte = fabsf(l.cte);
    float* s = p.stats + (size_t)i * kDaggerStatFloats;
    s[trsim::kDaggerStatTicks] = s[trsim::kDaggerStatTicks] + 1.0f;
    s[trsim::kDaggerStatExpertTicks] = s[trsim::kDaggerStatExpertTicks] + (expert ? 1.0f : 0.0f);
    s[trsim::kDaggerStatSumAbsCte] = s[trsim::kDaggerStatSumAbsCte] + acte;
    s[trsim::kDaggerStatMaxAbsCte] = fmaxf(s[trsim::kDaggerStatMaxAbsCte], acte);
    s[trsim::kDaggerStatSumAbsDiff] = s[trsim::kDaggerStatSumAbsDiff] + fabsf(ps - l.steer);
    s[trsim::kDaggerStatDone] = s[trsim::kDaggerStatDone] + (p.rule.done[i] ? 1.0f : 0.0f);
}

// what trs_set_expert keeps per handle (behind trs_internal_expert_slot); its buffers are the project's owning type
struct ExpertCtx {
    trs_expert_config cfg{};
    trsim::DevBuf<float> track_yaw, profile, target, w;
    trsim::DevBuf<float> stats;         // float[n][6] of trs_step_dagger (trs_dagger_stats)
    bool has_profile = false;
    int n = 0, n_points = 0;
    uint32_t k = 0;                     // ticks driven since trs_set_expert (trs_step_expert and trs_step_dagger share it)
};

ExpertRule rule_of(const trs_env* e, const ExpertCtx* c)
{
    ExpertRule r{};
    r.seg_idx = e->pp.seg_idx; r.yaw = e->pp.yaw; r.cte = e->pp.cte; r.speed = e->pp.speed; r.done = e->pp.done;
    r.track_yaw = c->track_yaw.get(); r.profile = c->has_profile ? c->profile.get() : nullptr; r.target = c->target.get();
    r.np = c->n_points; r.look = c->cfg.look;
    r.k_cte = c->cfg.k_cte; r.k_head = c->cfg.k_head; r.thr_hi = c->cfg.thr_hi; r.thr_lo = c->cfg.thr_lo;
    r.brake_over = c->cfg.brake_over; r.brake_val = c->cfg.brake_val;
    return r;
}

ExpertParams params_of(const trs_env* e, const ExpertCtx* c, int n)
{
    ExpertParams p{};
    p.rule = rule_of(e, c);
    p.n = n; p.env_id_base = e->cfg.env_id_base;
    p.alpha = c->cfg.alpha; p.sigma = c->cfg.sigma;
    p.seed = c->cfg.seed; p.k = c->k;
    return p;
}

// every launch of the two label kernels: one thread per env, on the view's stream
template <class P>
int launch_label(void (*kernel)(P), hipStream_t stream, const P& p)
{
    hipLaunchKernelGGL(kernel, dim3((p.n + 255) / 256), dim3(256), 0, stream, p);
    HIPCHK(hipGetLastError());
    return TRS_OK;
}

// how every entry point behind trs_set_expert begins: the handle's driver
int enter(trs_env* e, ExpertCtx** c)
{
    if (!e) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    *c = static_cast<ExpertCtx*>(*trs_internal_expert_slot(e));
    if (!*c) return trs_internal_fail(TRS_ERR_STATE, "no expert set (trs_set_expert)");
    return TRS_OK;
}

// what the ops of the two labelling loops share (trsim_loop.hpp): the driver, and where the row of a captured tick goes
struct LabelOps : TrsLoopOps {
    ExpertCtx* c;
    float* rows(int slot) const { return slot >= 0 ? cap->d_rows + (size_t)slot * e->n * kExpertRowFloats : nullptr; }
};

// trs_step_expert: the expert drives.  The frame of a record is the rendered truth of the state the label is computed on, whatever the latency or codec
struct ExpertOps : LabelOps {
    int observe(const uint8_t** frame) { int rc = trs_internal_tick_view(e, &v); if (!rc) *frame = v.latest_frame; return rc; }
    int label(int slot)
    {
        ExpertParams p = params_of(e, c, e->n);
        p.w = c->w.get();                                    // the disturbance state moves: closed_loop moves the counter with it
        p.out_steer = v.ctl_steer; p.out_thr = v.ctl_thr; p.out_brk = v.ctl_brk;
        p.rows = rows(slot);
        return launch_label(trs_expert_kernel, v.stream, p);
    }
};

// trs_step_dagger: the pilot acts, the expert labels the truth, the gate decides.  The frame of a record is the one the pilot was fed (the latest frame, the
// delay line's, the codec buffer's; nullptr: none exists yet, its controls are zero)
struct DaggerOps : LabelOps {
    const trs_pilot_config* pilot_cfg; const trs_dagger_config* cfg;
    int observe(const uint8_t** fed) { return trs_internal_pilot_tick(e, pilot_cfg, &v, fed); }
    int label(int slot)
    {
        DaggerParams p{};
        p.rule = rule_of(e, c);
        p.ctl_steer = v.ctl_steer; p.ctl_thr = v.ctl_thr; p.ctl_brk = v.ctl_brk;
        p.rows = rows(slot);
        p.stats = c->stats.get();                            // the stats move: closed_loop moves the counter with them
        p.n = e->n; p.env_id_base = e->cfg.env_id_base; p.expert_speed = cfg->expert_speed;
        p.beta = cfg->beta; p.seed = cfg->seed; p.block = c->k / (uint32_t)cfg->hold;
        return launch_label(trs_dagger_kernel, v.stream, p);
    }
};

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
    HIPCHK(c->stats.alloc((size_t)e->n * kDaggerStatFloats * 4));
    if (h_profile) HIPCHK(c->profile.alloc((size_t)np * 4));
    HIPCHK(hipMemcpy(c->track_yaw.get(), ty.data(), (size_t)np * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->target.get(), tg.data(), (size_t)e->n * 4, hipMemcpyHostToDevice));
    if (h_profile) HIPCHK(hipMemcpy(c->profile.get(), h_profile, (size_t)np * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(c->w.get(), 0, (size_t)e->n * 4));
    HIPCHK(hipMemset(c->stats.get(), 0, (size_t)e->n * kDaggerStatFloats * 4));
    trs_internal_count(e, 0, (size_t)np * 4 * (h_profile ? 2 : 1) + (size_t)e->n * 4);
    trs_expert_free(*slot);
    *slot = c;
    guard.c = nullptr;
    return TRS_OK;
}

TRS_EXPORT int trs_expert_act(trs_env* e, float* d_steer, float* d_thr, float* d_brk, int n)
{
    ExpertCtx* c;
    if (int rc = enter(e, &c)) return rc;
    if (!d_steer || !d_thr || !d_brk || n < 0 || n > e->n) return trs_internal_fail(TRS_ERR_ARG, "null output or n out of range (n <= n_envs)");
    HIPCHK(hipSetDevice(e->device));
    if (n == 0) return TRS_OK;
    { int rq = trsim::quiesce_handle(e); if (rq) return rq; }   // the kernel goes onto the handle's stream and reads the state behind the posted steps
    ExpertParams p = params_of(e, c, n);
    p.out_steer = d_steer; p.out_thr = d_thr; p.out_brk = d_brk;
    int rc = launch_label(trs_expert_kernel, e->sP, p);
    if (!rc) trsim::resident_note_launch(e);                 // resident mode selected: this kernel has no completion flag, trs_sync waits for the stream
    return rc;
}

TRS_EXPORT int trs_step_expert(trs_env* e, int n_steps, const trs_expert_capture* cap, int* n_captured)
{
    ExpertCtx* c;
    if (int rc = enter(e, &c)) return rc;
    if (n_steps < 1) return trs_internal_fail(TRS_ERR_ARG, "n_steps < 1");
    if (const char* why = trsim::expert_capture_error(cap, e->cfg.render != 0)) return trs_internal_fail(TRS_ERR_ARG, why);
    HIPCHK(hipSetDevice(e->device));
    ExpertOps ops{{{e, cap, {}}, c}};
    return trsim::closed_loop(ops, n_steps, cap, &c->k, n_captured);
}

// ---- pilot in the loop with the expert's labels (include/trsim_spec.h) ----
TRS_EXPORT void trs_default_dagger_config(trs_dagger_config* cfg)
{
    if (cfg) trsim::dagger_defaults(cfg);
}

TRS_EXPORT int trs_step_dagger(trs_env* e, const trs_pilot_config* pilot_cfg, const trs_dagger_config* cfg, int n_steps, const trs_expert_capture* cap, int* n_captured)
{
    ExpertCtx* c;
    if (int rc = enter(e, &c)) return rc;
    { int rp = trs_internal_pilot_loop_check(e, pilot_cfg, n_steps); if (rp) return rp; }    // trs_step_pilot's own refusals
    if (const char* why = trsim::dagger_config_error(cfg)) return trs_internal_fail(TRS_ERR_ARG, why);
    if (const char* why = trsim::expert_capture_error(cap, e->cfg.render != 0)) return trs_internal_fail(TRS_ERR_ARG, why);
    HIPCHK(hipSetDevice(e->device));
    DaggerOps ops{{{e, cap, {}}, c}, pilot_cfg, cfg};
    return trsim::closed_loop(ops, n_steps, cap, &c->k, n_captured);
}

TRS_EXPORT int trs_dagger_stats(trs_env* e, float* h_out, const float** d_out, int reset)
{
    ExpertCtx* c;
    if (int rc = enter(e, &c)) return rc;
    HIPCHK(hipSetDevice(e->device));
    const size_t bytes = (size_t)c->n * kDaggerStatFloats * sizeof(float);
    if (d_out) *d_out = c->stats.get();
    if (!h_out && !reset) return TRS_OK;
    { int rq = trsim::quiesce_handle(e); if (rq) return rq; }   // the copy and the reset go onto the handle's stream, behind the ticks queued so far
    if (h_out) {
        HIPCHK(hipMemcpyAsync(h_out, c->stats.get(), bytes, hipMemcpyDeviceToHost, e->sP));
        trs_internal_count(e, bytes, 0);
    }
    if (reset) HIPCHK(hipMemsetAsync(c->stats.get(), 0, bytes, e->sP));
    if (h_out) HIPCHK(hipStreamSynchronize(e->sP));
    trsim::resident_note_launch(e);                          // resident mode selected: stream work without a completion flag, trs_sync waits for the stream
    return TRS_OK;
}
