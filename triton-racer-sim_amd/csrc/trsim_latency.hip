// trsim_latency.hip — observation latency of libtrsim.so (include/trsim_spec.h, "observation latency"): trs_obs_kernel, the one launch behind every step
// while a latency is set, and trs_set_latency / trs_get_latency / trs_get_observation.  What the handle keeps is one ObsHistory (trsim_latency.hpp); the
// step paths of trsim_hip.hip reach this unit through launch_obs, latency_restart and obs_view (trsim_env.hpp), and trs_fetch_observation lies there
// beside trs_fetch_outputs, whose staging it shares.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>

#include "../../include/trsim.h"
#include "trsim_env.hpp"
#include "trsim_internal.hpp"

namespace {

// Workgroups [0, tel_blocks): one thread per env files the step's telemetry in ring slot `slot_now` and gathers the env's delayed record (zeros and
// arrived = 0 until it exists).  The other workgroups (only when the envs' delays differ) move every env's delayed frame, then depth frame, from its ring
// slot into the gathered frame: a copy, 16 B per lane, kObsVecs loads in flight per thread, the source slot uniform per workgroup, no LDS.  Source and
// destination lie at the same offset from a 256-aligned base, so one split serves both: up to three 4-byte pieces in front of the 16-aligned middle
// (an env's frame is a multiple of 4 bytes, of 16 only for some sizes) and up to three behind it.  Envs that have not arrived get zeros without a read.
constexpr int kObsBlock = 256, kObsVecs = 4;
struct ObsFrames { const uint8_t* ring; size_t stride; uint8_t* out; unsigned env_bytes; int blocks_per_env; };
struct ObsParams {
    const float* truth[5]; const int32_t* seg;                // x y z speed cte | seg_idx as the step left them
    float* ring_tel;                                          // [slots][6][n]
    const int32_t* ticks;                                     // L_e
    float* out_tel; uint8_t* out_flag;                        // [6][n] | arrived[n], mode[n]
    int n, slots, slot_now;
    long long T;                                              // steps of the history so far, this one included
    int tel_blocks;
    ObsFrames img, dep;                                       // blocks_per_env == 0: nothing to gather
};
// workgroups per env frame: 16 KiB of the middle each, at least one (it also moves the 4-byte pieces)
inline int obs_blocks_per_env(unsigned env_bytes) { const unsigned per = kObsBlock * kObsVecs; return (int)std::max(1u, (env_bytes / 16u + per - 1) / per); }

// Has the record an env with delay L is told after this step been filed, and the ring slot it lies in (ObsRing's arithmetic in 32 bits: 0 <= L < slots) —
// for the telemetry thread and for the frame mover alike.  Two value-returning functions, not one with an out-parameter or a pair: those forms were
// compiled and schedule the kernel differently; these leave its instructions as they were with the arithmetic written out twice (scripts/kernel_diff.py).
__device__ __forceinline__ bool obs_arrived(const ObsParams& p, int L) { return p.T - (long long)L >= 1; }
__device__ __forceinline__ int obs_slot(const ObsParams& p, int L)
{
    int slot = p.slot_now - L;
    if (slot < 0) slot += p.slots;
    return slot;
}

__device__ __forceinline__ void obs_move_env(const ObsFrames& f, const ObsParams& p, int env, int blk, int tid)
{
    const int L = p.ticks[env];
    const bool arrived = obs_arrived(p, L);
    const int slot = obs_slot(p, L);
    const size_t off = (size_t)env * f.env_bytes;
    const unsigned head = min((16u - (unsigned)(off & 15u)) & 15u, f.env_bytes);
    const unsigned vecs = (f.env_bytes - head) >> 4, tail = f.env_bytes - head - (vecs << 4);
    const uint8_t* const src = f.ring + (size_t)slot * f.stride + off;
    uint8_t* const dst = f.out + off;
    const uint4* const s4 = reinterpret_cast<const uint4*>(src + head);
    uint4* const d4 = reinterpret_cast<uint4*>(dst + head);
    const unsigned v0 = (unsigned)blk * (kObsBlock * kObsVecs) + (unsigned)tid;
    uint4 r[kObsVecs];
#pragma unroll
    for (int k = 0; k < kObsVecs; ++k) {
        const unsigned i = v0 + k * kObsBlock;
        r[k] = make_uint4(0u, 0u, 0u, 0u);
        if (arrived && i < vecs) r[k] = s4[i];
    }
#pragma unroll
    for (int k = 0; k < kObsVecs; ++k) {
        const unsigned i = v0 + k * kObsBlock;
        if (i < vecs) d4[i] = r[k];
    }
    if (blk == 0) {                                           // the 4-byte pieces: threads 0..2 in front, 64..66 behind
        const unsigned t = (unsigned)tid;
        if (t < head / 4u) reinterpret_cast<uint32_t*>(dst)[t] = arrived ? reinterpret_cast<const uint32_t*>(src)[t] : 0u;
        const unsigned tb = head + (vecs << 4);
        if (t >= 64u && t - 64u < tail / 4u)
            reinterpret_cast<uint32_t*>(dst + tb)[t - 64u] = arrived ? reinterpret_cast<const uint32_t*>(src + tb)[t - 64u] : 0u;
    }
}

__global__ __launch_bounds__(kObsBlock) void trs_obs_kernel(const ObsParams p)
{
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    if (b < p.tel_blocks) {
        const int i = b * kObsBlock + tid;
        if (i >= p.n) return;
        const size_t n = (size_t)p.n;
        float* const now = p.ring_tel + (size_t)p.slot_now * 6 * n;
#pragma unroll
        for (int k = 0; k < 5; ++k) now[k * n + i] = p.truth[k][i];
        reinterpret_cast<int32_t*>(now)[5 * n + i] = p.seg[i];
        const int L = p.ticks[i];
        const bool arrived = obs_arrived(p, L);
        const int slot = obs_slot(p, L);
        const float* const then = p.ring_tel + (size_t)slot * 6 * n;      // (L == 0: what this thread has just stored)
#pragma unroll
        for (int k = 0; k < 5; ++k) p.out_tel[k * n + i] = arrived ? (L == 0 ? p.truth[k][i] : then[k * n + i]) : 0.0f;
        reinterpret_cast<int32_t*>(p.out_tel)[5 * n + i] = arrived ? (L == 0 ? p.seg[i] : reinterpret_cast<const int32_t*>(then)[5 * n + i]) : 0;
        p.out_flag[i] = arrived ? 1 : 0;
        p.out_flag[n + i] = arrived ? (uint8_t)TRS_MODE_AI : (uint8_t)TRS_MODE_HUMAN;
        return;
    }
    b -= p.tel_blocks;
    const int img_blocks = p.n * p.img.blocks_per_env;
    if (b < img_blocks) { obs_move_env(p.img, p, b / p.img.blocks_per_env, b % p.img.blocks_per_env, tid); return; }
    b -= img_blocks;
    if (p.dep.blocks_per_env > 0 && b < p.n * p.dep.blocks_per_env) obs_move_env(p.dep, p, b / p.dep.blocks_per_env, b % p.dep.blocks_per_env, tid);
}

trsim::ObsBytes bytes_of(const trs_env* e, const trsim::ObsRing& ring) { return trsim::obs_bytes(ring, e->n, e->H, e->W, e->cfg.render != 0, e->cfg.depth != 0); }

}  // namespace

// The launch behind every step while an observation latency is set (trs_obs_kernel): the step that has just been counted is filed in the ring and every
// env's delayed record gathered.  One delay for all envs: the frame view points into the ring (obs_view) and only the telemetry part runs.
int trsim::launch_obs(trs_env* e)
{
    const ObsHistory& h = e->obs;
    const long long T = h.steps(e->step_count);
    const PParams& k = e->pp;
    ObsParams p;
    std::memset(&p, 0, sizeof p);
    p.truth[0] = k.x; p.truth[1] = k.y; p.truth[2] = k.z; p.truth[3] = k.speed; p.truth[4] = k.cte; p.seg = k.seg_idx;
    p.ring_tel = h.ring_tel.get(); p.ticks = h.ticks.get();
    const int b = ObsRing::gather_buf(T);
    p.out_tel = h.tel[b].get(); p.out_flag = h.flag[b].get();
    p.n = e->n; p.slots = h.ring.slots(); p.slot_now = h.ring.slot_of_step(T); p.T = T;
    p.tel_blocks = (e->n + kObsBlock - 1) / kObsBlock;
    int grid = p.tel_blocks;
    if (e->cfg.render && !h.uniform) {
        const ObsBytes sz = bytes_of(e, h.ring);
        p.img = ObsFrames{h.ring_img.get(), h.img_stride, e->img[b].get(), (unsigned)sz.img_env, 0};
        p.img.blocks_per_env = obs_blocks_per_env(p.img.env_bytes);
        grid += e->n * p.img.blocks_per_env;
        if (e->cfg.depth) {
            p.dep = ObsFrames{reinterpret_cast<const uint8_t*>(h.ring_dep.get()), h.dep_stride, reinterpret_cast<uint8_t*>(e->depth[b].get()), (unsigned)sz.dep_env, 0};
            p.dep.blocks_per_env = obs_blocks_per_env(p.dep.env_bytes);
            grid += e->n * p.dep.blocks_per_env;
        }
    }
    hipLaunchKernelGGL(trs_obs_kernel, dim3(grid), dim3(kObsBlock), 0, e->sP, p);
    HIPCHK(hipGetLastError());
    return TRS_OK;
}

// The history of observations begins (trs_set_latency, trs_load_track): nothing has arrived, and every slot an observation can point into before a step
// has written it holds the constructor's state.  The handle's stream is idle when this is called.
int trsim::latency_restart(trs_env* e)
{
    ObsHistory& h = e->obs;
    h.base = e->step_count;
    if (h.ring_img.get()) HIPCHK(hipMemsetAsync(h.ring_img.get(), 0, h.ring_img.bytes(), e->sP));
    if (h.ring_dep.get()) HIPCHK(hipMemsetAsync(h.ring_dep.get(), 0, h.ring_dep.bytes(), e->sP));
    for (int b = 0; b < 2; ++b) {
        HIPCHK(hipMemsetAsync(h.tel[b].get(), 0, h.tel[b].bytes(), e->sP));
        HIPCHK(hipMemsetAsync(h.flag[b].get(), 0, h.flag[b].bytes(), e->sP));
        if (!h.uniform && e->img[b].get()) HIPCHK(hipMemsetAsync(e->img[b].get(), 0, e->img[b].bytes(), e->sP));        // the gathered frames
        if (!h.uniform && e->depth[b].get()) HIPCHK(hipMemsetAsync(e->depth[b].get(), 0, e->depth[b].bytes(), e->sP));
    }
    HIPCHK(hipStreamSynchronize(e->sP));
    return TRS_OK;
}

// what the car is told after the last step (trs_get_observation): device pointers into the gathered telemetry and, for the frames, into the ring (one
// delay for all envs: no frame byte is moved) or the gathered frames
void trsim::obs_view(const trs_env* e, trs_obs_view* o)
{
    const ObsHistory& h = e->obs;
    const long long T = h.steps(e->step_count);
    const int b = ObsRing::gather_buf(T);
    const size_t n = (size_t)e->n;
    const float* t = h.tel[b].get();
    o->struct_size = (uint32_t)sizeof *o;
    o->n_envs = e->n; o->img_h = e->H; o->img_w = e->W;
    o->img = nullptr; o->depth = nullptr;
    if (e->cfg.render) {
        const int slot = h.ring.slot_of_obs(T, h.all);
        o->img = h.uniform ? h.frame(slot) : e->img[b].get();
        if (e->cfg.depth) o->depth = h.uniform ? h.depth(slot) : e->depth[b].get();
    }
    o->pos_x = t; o->pos_y = t + n; o->pos_z = t + 2 * n; o->speed = t + 3 * n; o->cte = t + 4 * n;
    o->seg_idx = reinterpret_cast<const int32_t*>(t + 5 * n);
    o->arrived = h.flag[b].get();
}

TRS_EXPORT int trs_set_latency(trs_env* e, const int32_t* h_ticks, int max_ticks)
{
    if (!e) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    if (h_ticks) {
        if (max_ticks < 1 || max_ticks > trsim::kMaxLatencyTicks) return trs_internal_fail(TRS_ERR_ARG, "max_ticks must be in [1, " + std::to_string(trsim::kMaxLatencyTicks) + "]");
        for (int i = 0; i < e->n; ++i)
            if (h_ticks[i] < 0 || h_ticks[i] > max_ticks) return trs_internal_fail(TRS_ERR_ARG, "the latency of env " + std::to_string(i) + " is " + std::to_string(h_ticks[i]) + " ticks: outside [0, max_ticks = " + std::to_string(max_ticks) + "]");
        if (trsim::resident_selected(e))
            return trs_internal_fail(TRS_ERR_STATE, "resident mode is selected (trs_set_step_mode): the worker's frame hand-off is built on two buffers by step parity, an observation latency needs "
                                                    "steps by launches (TRS_STEP_LAUNCH first)");
    }
    HIPCHK(hipSetDevice(e->device));
    int rc = trsim::sync_handle(e);
    if (rc) return rc;
    if (!h_ticks) {                                          // off: back to the two frame buffers; the next step into each stores a whole frame
        if (!e->obs.on()) return TRS_OK;
        e->obs = trsim::ObsHistory{};
        e->uniform_ok.invalidate();
        return TRS_OK;
    }
    // everything the new setting needs is allocated first: a failure leaves the handle as it was
    trsim::ObsHistory next;
    next.ring.max_ticks = max_ticks;
    const trsim::ObsBytes sz = bytes_of(e, next.ring);
    const size_t n = (size_t)e->n;
    auto want = [&](auto& buf, size_t bytes) -> int {
        if (!bytes) return TRS_OK;
        const hipError_t rh = buf.alloc(bytes);
        if (rh == hipSuccess) return TRS_OK;
        (void)hipGetLastError();
        return trs_internal_fail(rh == hipErrorOutOfMemory ? TRS_ERR_NOMEM : TRS_ERR_DEVICE,
                                 "trs_set_latency: the observation ring of " + std::to_string(next.ring.slots()) + " slots wanted " + std::to_string(bytes) + " bytes of device memory (" + hipGetErrorString(rh) + "); the handle is unchanged");
    };
    if ((rc = want(next.ring_img, sz.ring_img)) || (rc = want(next.ring_dep, sz.ring_dep)) || (rc = want(next.ring_tel, sz.ring_tel)) || (rc = want(next.ticks, sz.ticks))) return rc;
    for (int b = 0; b < 2; ++b)
        if ((rc = want(next.tel[b], sz.tel)) || (rc = want(next.flag[b], sz.flag))) return rc;
    HIPCHK(hipMemcpy(next.ticks.get(), h_ticks, sz.ticks, hipMemcpyHostToDevice));
    e->h2d_bytes += sz.ticks;
    next.img_stride = sz.img_stride; next.dep_stride = sz.dep_stride;
    next.host.assign(h_ticks, h_ticks + n);
    next.all = h_ticks[0];
    next.uniform = std::all_of(h_ticks, h_ticks + n, [&](int32_t t) { return t == h_ticks[0]; });
    e->obs = std::move(next);                                // commit: the old setting's buffers are released here (the stream is idle)
    e->uniform_ok.invalidate();                              // img[] / depth[] become the gathered frames (or lie idle): no step has claimed them when the latency goes off again
    return trsim::latency_restart(e);
}

TRS_EXPORT int trs_get_latency(trs_env* e, int32_t* h_ticks_out, int* max_ticks_out)
{
    if (!e) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    if (max_ticks_out) *max_ticks_out = e->obs.ring.max_ticks;
    if (h_ticks_out)
        for (int i = 0; i < e->n; ++i) h_ticks_out[i] = e->obs.on() ? e->obs.host[(size_t)i] : 0;
    return TRS_OK;
}

TRS_EXPORT int trs_get_observation(trs_env* e, trs_obs_view* out)
{
    if (!e || !out) return trs_internal_fail(TRS_ERR_ARG, "null argument");
    if (!e->obs.on()) return trs_internal_fail(TRS_ERR_STATE, "no observation latency is set (trs_set_latency): the observation is the state, trs_get_state");
    trsim::obs_view(e, out);
    return TRS_OK;
}
