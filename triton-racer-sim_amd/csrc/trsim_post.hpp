// trsim_post.hpp — the host's half of the resident worker's post protocol, and nothing of HIP: the layout of the pinned mailbox and its codes,
// the host's ledger of what it has posted and seen complete (PostLedger), the post itself, and the pinned staging slot of host-array controls.
// trsim_resident.hip includes it for its kernels (the layout, the codes) and for its host side, which keeps the ACTIONS — launching a worker,
// waiting, evicting — and states every change of the bookkeeping through a transition named here.  Everything in this file can be decided
// without a GPU, so it is pinned on the CPU: tests/resident_post_driver.cpp (ASan + UBSan; its two-thread case under TSan).
#pragma once

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "trsim_plan.hpp"

namespace trsim {

// ---- the protocol's layout and codes ---------------------------------------------------------------------------------------------------------
constexpr int kSlots = 8;       // posts in flight: ring entries, arrival counters, done flags

struct WEntry {                 // one posted step: ONE 64-B line, so the dispatcher learns of a post and gets it in one PCIe read
    uint64_t seq_lo;            // step index + 1: the tag of the line's FIRST 32-byte half, written by the host after steer / thr / brk
    const float* steer; const float* thr; const float* brk;
    const uint8_t* reset;
    uint32_t synth, pad0;
    uint64_t seq;               // step index + 1, written LAST: the tag of the second half.  The line is a valid post for step s iff
                                // seq_lo == seq == s + 1 — should the device's 64-byte read ever be served as two 32-byte requests, a
                                // stale half cannot pair with a fresh one (each half carries its own tag, written after its payload)
    uint64_t pad1;
};
static_assert(sizeof(WEntry) == 64, "one entry per 64-B line");
constexpr int kTagLo = 0, kTagHi = 6;   // u64 word indices of the two tags within a line
static_assert(offsetof(WEntry, seq_lo) == 8 * kTagLo && offsetof(WEntry, seq) == 8 * kTagHi && offsetof(WEntry, reset) == 32, "tag placement");

struct Mailbox {                // pinned host memory the device reads and writes over PCIe
    alignas(64) uint64_t close;             // host -> device: leave once everything posted is done
    uint64_t posted;                        // host bookkeeping: steps [0, posted) have been posted (the device reads the entries' tags)
    alignas(64) uint64_t exited;            // device -> host: the dispatcher has decided to leave (kExitNormal), or it found the launch NOT co-resident
                                            //   (kExitNotCoresident: another worker — of another process — holds part of the CUs; nothing was consumed)
    uint64_t consumed;                      //   ... and every step below this index is processed by the time the kernel ends
    uint64_t error;                         //   non-zero: a bounded wait gave up (GiveUp code << 32 | block)
    uint64_t started;                       //   1 = every workgroup of this launch has reported in: the launch is co-resident and serves posts
    alignas(64) uint64_t done[kSlots];      // device -> host: done[s % 8] = s + 1 when step s is complete in memory
    alignas(64) WEntry ring[kSlots];        // host -> device
};

constexpr unsigned long long kExitNormal = 1ull, kExitNotCoresident = 2ull;     // Mailbox::exited
constexpr unsigned long long kCloseLeave = 1ull, kCloseCancel = 2ull;            // Mailbox::close: leave once everything posted is done / the host has given up on this launch
constexpr unsigned kRetryMs0 = 100;

// Mailbox::error's code: which bounded wait of the worker gave up (6 and 8 have never been used), and the host's text for each (worker_error)
enum GiveUp : unsigned { kGiveUpPost = 1, kGiveUpCamRing = 2, kGiveUpPhysics = 3, kGiveUpForward = 4, kGiveUpBarrier = 5, kGiveUpInjected = 7, kGiveUpLdsBase = 9 };
constexpr const char* kGiveUpText[10] = {"", "waiting for a post", "camera ring back-pressure", "waiting for the physics team", "forwarding the last arrivals",
                                         "team barrier of the dynamic-brightness batch", "", "abort injected by trs_resident_debug_abort (test hook)", "",
                                         "dynamic LDS segment not at offset 0"};
inline const char* give_up_text(unsigned code) { return code < 10 ? kGiveUpText[code] : "?"; }

inline uint64_t host_load(const uint64_t* p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }
inline void host_store(uint64_t* p, uint64_t v) { __atomic_store_n(p, v, __ATOMIC_RELEASE); }

// ---- the ledger ------------------------------------------------------------------------------------------------------------------------------
// What the host knows of a handle's resident mode.  The fields are read freely; they change through the transitions below and nowhere else.
struct PostLedger {
    using Clock = std::chrono::steady_clock;
    bool enabled = false;       // resident mode is selected and in use: step calls post
    bool running = false;       // a worker kernel of this handle is on the handle's stream (launched and not yet waited for)
    bool launched = false;      // steps were LAUNCHED on the handle's stream since the last wait (trs_step_pilot in resident mode, a fall-back's replay): no
                                // completion flag will ever be written for them — the stream is what to wait for
    bool fell_back = false;     // a launch of the worker was found not co-resident (another process's worker on the GPU): the handle went
                                // back to TRS_STEP_LAUNCH by itself (trs_last_error() says so); it selects resident mode again when retry_due
    bool broken = false;        // a worker gave up (bounded wait): some workgroups may have taken a step others did not — the env
                                // state is undefined until the track is loaded again; every resident call fails meanwhile
    uint64_t base = 0;          // steps [base, step_count) were handed to the worker since the last restart
    uint64_t seen_done = 0;     // every step below this index has been observed complete
    unsigned retry_ms = kRetryMs0;   // resident mode is tried again this long after t_fallback, doubling up to 2 s while the GPU stays shared
    Clock::time_point t_fallback{};

    // nothing is in flight that a flag will report: the ledger starts afresh at `step` (the step counter may have moved or restarted since)
    void restart(uint64_t step) { base = seen_done = step; }
    // ... and the launched steps are accounted for: the stream has been waited for, or they are ahead of the next worker on the same stream
    void absorb(uint64_t step) { launched = false; restart(step); }
    // a step went onto the stream as a launch: it has no post and gets no flag
    void note_launch(uint64_t step) { launched = true; restart(step); }
    // a done flag (index + 1) or the consumed count of a kernel that has ended: seen_done never runs backwards
    void observe(uint64_t count) { seen_done = std::max(seen_done, count); }
    // the ring holds posts nobody serves: an eviction by another handle left them behind, and no launched step has moved the counter since
    bool orphans(uint64_t posted, uint64_t step) const { return posted > seen_done && posted == step; }
    // ring slot, counters, done flag and staging slot of s % kSlots are still those of step s - kSlots: it must be seen done first
    bool must_wait(uint64_t s) const { return s >= base + kSlots; }
    void worker_launched() { running = true; }
    void worker_ended() { running = false; }
    void worker_had_the_gpu() { retry_ms = kRetryMs0; }     // a launch reported in: the sharing that caused an earlier fall-back is over
    void gave_up() { broken = true; }
    void clear_fault() { broken = false; }
    void fall_back(Clock::time_point now) { enabled = false; fell_back = true; t_fallback = now; }
    bool retry_due(Clock::time_point now) const { return !enabled && fell_back && !broken && now - t_fallback >= std::chrono::milliseconds(retry_ms); }
    // Selecting resident mode: by the caller (select) or by the handle itself after a fall-back (reselect, retry_due).  true: the mode was
    // off, the ledger has restarted at `step` and Mailbox::posted must follow it.
    bool select(uint64_t step) { retry_ms = kRetryMs0; return turn_on(step); }
    bool reselect(uint64_t step) { retry_ms = std::min(retry_ms * 2u, 2000u); launched = false; return turn_on(step); }
    void deselect() { enabled = false; }
private:
    bool turn_on(uint64_t step) { const bool was_off = !enabled; if (was_off) restart(step); enabled = true; fell_back = false; return was_off; }
};

// ---- the post --------------------------------------------------------------------------------------------------------------------------------
// Step s goes into its line of the ring: each half's payload, then that half's tag (x86 keeps the store order); the second tag makes the line
// a valid post, then the host's own count follows.
inline void write_post(Mailbox* mb, uint64_t s, const Controls& c)
{
    WEntry* slot = &mb->ring[s & (kSlots - 1)];
    slot->steer = c.steer; slot->thr = c.thr; slot->brk = c.brk;
    host_store(&slot->seq_lo, s + 1);
    slot->reset = c.reset; slot->synth = c.synth ? 1u : 0u;
    host_store(&slot->seq, s + 1);
    host_store(&mb->posted, s + 1);
}
inline bool whole_post(const WEntry& en, uint64_t s) { return en.seq == s + 1 && en.seq_lo == s + 1; }
// tags and flags of the past must not match a step index that comes round again
inline void forget_ring(Mailbox* mb) { for (int k = 0; k < kSlots; ++k) { host_store(&mb->ring[k].seq, 0); host_store(&mb->ring[k].seq_lo, 0); host_store(&mb->done[k], 0); } }

// ---- the staging of host-array controls ------------------------------------------------------------------------------------------------------
// Controls handed over as host arrays are read by the device from pinned memory: kSlots slots of float steer[n], thr[n], brk[n], uint8 reset[n],
// one per post in flight.  Held controls over several steps are carried from slot to slot, since the slot of a step is reused kSlots steps later.
constexpr size_t stage_offset(int array, size_t n) { return (size_t)array * 4 * n; }       // 0 steer, 1 thr, 2 brk, 3 reset
constexpr size_t stage_slot_bytes(size_t n) { return (stage_offset(3, n) + n + 63) & ~(size_t)63; }
inline unsigned char* stage_slot(unsigned char* staging, uint64_t s, size_t n) { return staging + (s & (kSlots - 1)) * stage_slot_bytes(n); }
inline void stage_fill(unsigned char* slot, const Controls& h, size_t n)
{
    std::memcpy(slot + stage_offset(0, n), h.steer, n * 4); std::memcpy(slot + stage_offset(1, n), h.thr, n * 4);
    if (h.brk) std::memcpy(slot + stage_offset(2, n), h.brk, n * 4);
    if (h.reset) std::memcpy(slot + stage_offset(3, n), h.reset, n);
}
inline void stage_carry(unsigned char* slot, const unsigned char* from, size_t n) { if (slot != from) std::memcpy(slot, from, stage_offset(3, n)); }
// what a step posted from `slot` reads: h's arrays there; no brake and no reset where h has none, the reset on the call's first step alone
inline Controls stage_controls(unsigned char* slot, const Controls& h, size_t n, bool first_step)
{
    const float* f = reinterpret_cast<const float*>(slot);
    return {f, f + n, h.brk ? f + 2 * n : nullptr, first_step && h.reset ? slot + stage_offset(3, n) : nullptr, 0, 0};
}

}  // namespace trsim
