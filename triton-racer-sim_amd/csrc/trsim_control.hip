// trsim_control.hip — the per-car control glue of libtrsim.so: DriverAssistance.step (trs_driver_assist) and ControlMultiplexer.step (trs_control_mux)
// for N cars, with their _host staging through the handle's glue buffer.  The handle is reached as in the JPEG units: trsim_env.hpp and the accessors
// of trsim_internal.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/trsim.h"
#include "trsim_env.hpp"
#include "trsim_internal.hpp"

namespace {

// DriverAssistance.step for N cars (components/driver_assistance.py:13-31), in place; binary64 like the reference's Python floats
__global__ void trs_driver_assist_kernel(int mode, double k, float* st, float* th, float* br, const float* sp, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double steering = st[i], throttle = th[i], breaking = br[i];
    const double speed = sp[i];
    if (mode == 0 && speed != 0) {
        const double max_steering = k / speed;
        if (steering > max_steering) { steering = max_steering; throttle = -0.1; }
        else if (steering < max_steering * -1) { steering = max_steering * -1; throttle = -0.1; }
    } else if (mode == 1 && steering != 0) {
        const double max_speed = k / steering;
        if (speed > max_speed) { throttle = 0.0; breaking = 0.0; }
    }
    st[i] = (float)steering; th[i] = (float)throttle; br[i] = (float)breaking;
}

// ControlMultiplexer.step for N cars (components/controlmultiplexer.py:24-43); semantics in include/trsim.h.
// Per-car state: int32 st[10] = 8 pending trigger ticks | ring head | last_mode + (steering lock << 8) + (throttle lock << 16)
constexpr int kMuxWords = 10;
constexpr int kMuxNone = INT32_MIN / 2;
struct MuxParams {
    const uint8_t* mode;
    const float *us, *ut, *ub, *as, *at, *ab;
    float *os, *ot, *ob;
    int32_t* state;
    int n, tick;
    int en_t, ticks_t, en_s, ticks_s;
    float val_t, val_s;
};

__global__ void trs_control_mux_kernel(const MuxParams p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n) return;
    int32_t* st = p.state + (size_t)i * kMuxWords;
    int flags = st[9];
    int last_mode = flags & 255, act_s = (flags >> 8) & 1, act_t = (flags >> 16) & 1;
    // lock-end threads whose sleep elapses at this tick run before the step (:51-54, :67-70)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int trig = st[j];
        if (p.en_t && trig + p.ticks_t == p.tick) act_t = 0;
        if (p.en_s && trig + p.ticks_s == p.tick) act_s = 0;
    }
    const int mode = p.mode[i];
    float s = 0.f, t = 0.f, b = 0.f;
    const bool known = mode <= TRS_MODE_AI;
    if (mode == TRS_MODE_HUMAN) { s = p.us[i]; t = p.ut[i]; b = p.ub[i]; }                    // :26-27
    else if (mode == TRS_MODE_AI_STEERING) { s = p.as[i]; t = p.ut[i]; b = p.ub[i]; }         // :28-29
    else if (mode == TRS_MODE_AI) { s = p.as[i]; t = p.at[i]; b = p.ab[i]; }                  // :30-31
    if (last_mode != TRS_MODE_AI && mode == TRS_MODE_AI && (p.en_t || p.en_s)) {             // :33-35 AI launch detection
        if (p.en_t) act_t = 1;
        if (p.en_s) act_s = 1;
        const int head = st[8];
        st[head & 7] = p.tick;
        st[8] = head + 1;
    }
    if (known) {
        if (act_s) s = p.val_s;                                                               // :37-38
        if (act_t) t = p.val_t;                                                               // :39-40
        p.os[i] = s; p.ot[i] = t; p.ob[i] = b;
    }
    st[9] = (mode & 255) | (act_s << 8) | (act_t << 16);                                      // :42
}

__global__ void trs_control_mux_init_kernel(int32_t* state, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int32_t* st = state + (size_t)i * kMuxWords;
    for (int j = 0; j < 8; ++j) st[j] = kMuxNone;
    st[8] = 0; st[9] = TRS_MODE_HUMAN;
}

// ---- host side ----

// device scratch of the *_host control glue, owned by the handle (the N = 1 Car loop calls these every tick)
int ensure_glue(trs_env* e, size_t bytes)
{
    if (bytes <= e->glue.bytes()) return TRS_OK;
    int rc = trsim::sync_handle(e);
    if (rc) return rc;
    HIPCHK(e->glue.reserve(std::max<size_t>(trsim::align_up(bytes, 256), 4096)));
    return TRS_OK;
}

}  // namespace

TRS_EXPORT int trs_driver_assist(trs_env* e, int mode, double k, float* d_st, float* d_th, float* d_br, const float* d_sp, int n)
{
    if (!e || !d_st || !d_th || !d_br || n < 0 || (mode != 0 && mode != 1)) return trs_internal_fail(TRS_ERR_ARG, "bad argument (mode 0 = steering, 1 = speed)");
    if (!d_sp) { if (n != e->n) return trs_internal_fail(TRS_ERR_ARG, "the env's own speed needs n == n_envs"); d_sp = e->pp.speed; }
    HIPCHK(hipSetDevice(e->device));
    if (n == 0) return TRS_OK;
    { int rq = trsim::quiesce_handle(e); if (rq) return rq; }
    hipLaunchKernelGGL(trs_driver_assist_kernel, dim3((n + 255) / 256), dim3(256), 0, e->sP, mode, k, d_st, d_th, d_br, d_sp, n);
    HIPCHK(hipGetLastError());
    return TRS_OK;
}

TRS_EXPORT int trs_driver_assist_host(trs_env* e, int mode, double k, float* h_st, float* h_th, float* h_br, const float* h_sp, int n)
{
    if (!e || !h_st || !h_th || !h_br || !h_sp || n < 0) return trs_internal_fail(TRS_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(e->device));
    if (n == 0) return TRS_OK;
    int rc = trsim::quiesce_handle(e);
    if (!rc) rc = ensure_glue(e, (size_t)n * 16);
    if (rc) return rc;
    float* d = e->glue.get();
    float *ds = d, *dt = d + n, *db = d + 2 * (size_t)n, *dp = d + 3 * (size_t)n;
    hipError_t err = hipSuccess;
    const float* srcs[4] = {h_st, h_th, h_br, h_sp};
    float* dsts[4] = {ds, dt, db, dp};
    for (int a = 0; a < 4 && err == hipSuccess; ++a) err = hipMemcpyAsync(dsts[a], srcs[a], (size_t)n * 4, hipMemcpyHostToDevice, e->sP);
    rc = err == hipSuccess ? trs_driver_assist(e, mode, k, ds, dt, db, dp, n) : trs_internal_fail(TRS_ERR_DEVICE, hipGetErrorString(err));
    float* outs[3] = {h_st, h_th, h_br};
    for (int a = 0; a < 3 && rc == TRS_OK; ++a)
        if (hipMemcpyAsync(outs[a], dsts[a], (size_t)n * 4, hipMemcpyDeviceToHost, e->sP) != hipSuccess) rc = trs_internal_fail(TRS_ERR_DEVICE, "copy back failed");
    if (hipStreamSynchronize(e->sP) != hipSuccess && rc == TRS_OK) rc = trs_internal_fail(TRS_ERR_DEVICE, "stream synchronisation failed");
    return rc;
}

TRS_EXPORT void trs_default_mux_config(trs_mux_config* c)
{
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = sizeof(*c);
    c->throttle_lock_enabled = 0; c->throttle_lock_value = 1.0f; c->throttle_lock_ticks = 100;   // core/config.py:57-59 at 20 Hz
    c->steering_lock_enabled = 0; c->steering_lock_value = 0.0f; c->steering_lock_ticks = 60;    // core/config.py:61-63
}

static int mux_state_ready(trs_env* e)
{
    { int rq = trsim::quiesce_handle(e); if (rq) return rq; }
    if (e->mux_state.get()) return TRS_OK;
    HIPCHK(e->mux_state.alloc((size_t)e->n * kMuxWords * sizeof(int32_t)));
    hipLaunchKernelGGL(trs_control_mux_init_kernel, dim3((e->n + 255) / 256), dim3(256), 0, e->sP, e->mux_state.get(), e->n);
    HIPCHK(hipGetLastError());
    e->mux_tick = 0;
    return TRS_OK;
}

TRS_EXPORT int trs_control_mux_reset(trs_env* e)
{
    if (!e) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(e->device));
    { int rq = trsim::quiesce_handle(e); if (rq) return rq; }
    HIPCHK(e->mux_state.reset());
    return mux_state_ready(e);
}

TRS_EXPORT int trs_control_mux(trs_env* e, const trs_mux_config* c, const uint8_t* d_mode, const float* d_us, const float* d_ut, const float* d_ub,
                               const float* d_as, const float* d_at, const float* d_ab, float* d_os, float* d_ot, float* d_ob, int n)
{
    if (!e || !c || !d_mode || !d_us || !d_ut || !d_ub || !d_as || !d_at || !d_ab || !d_os || !d_ot || !d_ob) return trs_internal_fail(TRS_ERR_ARG, "null argument");
    if (c->struct_size != sizeof(trs_mux_config)) return trs_internal_fail(TRS_ERR_ARG, "trs_mux_config.struct_size mismatch");
    if (n < 0 || n > e->n) return trs_internal_fail(TRS_ERR_ARG, "n must be in [0, n_envs] (the lock state is kept per env)");
    if ((c->throttle_lock_enabled && c->throttle_lock_ticks < 1) || (c->steering_lock_enabled && c->steering_lock_ticks < 1))
        return trs_internal_fail(TRS_ERR_ARG, "lock ticks must be >= 1");
    HIPCHK(hipSetDevice(e->device));
    int rc = mux_state_ready(e);
    if (rc) return rc;
    MuxParams p{};
    p.mode = d_mode; p.us = d_us; p.ut = d_ut; p.ub = d_ub; p.as = d_as; p.at = d_at; p.ab = d_ab; p.os = d_os; p.ot = d_ot; p.ob = d_ob;
    p.state = e->mux_state.get(); p.n = n; p.tick = e->mux_tick;
    p.en_t = c->throttle_lock_enabled != 0; p.ticks_t = c->throttle_lock_ticks; p.val_t = c->throttle_lock_value;
    p.en_s = c->steering_lock_enabled != 0; p.ticks_s = c->steering_lock_ticks; p.val_s = c->steering_lock_value;
    if (n > 0) {
        hipLaunchKernelGGL(trs_control_mux_kernel, dim3((n + 255) / 256), dim3(256), 0, e->sP, p);
        HIPCHK(hipGetLastError());
    }
    e->mux_tick += 1;
    return TRS_OK;
}

TRS_EXPORT int trs_control_mux_host(trs_env* e, const trs_mux_config* c, const uint8_t* h_mode, const float* h_us, const float* h_ut, const float* h_ub,
                                    const float* h_as, const float* h_at, const float* h_ab, float* h_os, float* h_ot, float* h_ob, int n)
{
    if (!e || !h_mode || !h_us || !h_ut || !h_ub || !h_as || !h_at || !h_ab || !h_os || !h_ot || !h_ob || n < 0) return trs_internal_fail(TRS_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(e->device));
    if (n == 0) return trs_control_mux(e, c, h_mode, h_us, h_ut, h_ub, h_as, h_at, h_ab, h_os, h_ot, h_ob, 0);
    const size_t nn = (size_t)n;
    int rc = trsim::quiesce_handle(e);
    if (!rc) rc = ensure_glue(e, nn * 4 * 9 + nn);
    if (rc) return rc;
    float* d = e->glue.get();
    uint8_t* dm = reinterpret_cast<uint8_t*>(d + 9 * nn);
    const float* srcs[9] = {h_us, h_ut, h_ub, h_as, h_at, h_ab, h_os, h_ot, h_ob};
    hipError_t err = hipMemcpyAsync(dm, h_mode, nn, hipMemcpyHostToDevice, e->sP);
    for (int a = 0; a < 9 && err == hipSuccess; ++a) err = hipMemcpyAsync(d + a * nn, srcs[a], nn * 4, hipMemcpyHostToDevice, e->sP);
    rc = err == hipSuccess ? trs_control_mux(e, c, dm, d, d + nn, d + 2 * nn, d + 3 * nn, d + 4 * nn, d + 5 * nn, d + 6 * nn, d + 7 * nn, d + 8 * nn, n)
                           : trs_internal_fail(TRS_ERR_DEVICE, hipGetErrorString(err));
    float* outs[3] = {h_os, h_ot, h_ob};
    for (int a = 0; a < 3 && rc == TRS_OK; ++a)
        if (hipMemcpyAsync(outs[a], d + (6 + a) * nn, nn * 4, hipMemcpyDeviceToHost, e->sP) != hipSuccess) rc = trs_internal_fail(TRS_ERR_DEVICE, "copy back failed");
    if (hipStreamSynchronize(e->sP) != hipSuccess && rc == TRS_OK) rc = trs_internal_fail(TRS_ERR_DEVICE, "stream synchronisation failed");
    return rc;
}
