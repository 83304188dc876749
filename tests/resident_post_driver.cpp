// Test driver (CPU): the host's half of the resident worker's post protocol (triton-racer-sim_amd/csrc/trsim_post.hpp, the header alone) printed for
// tests/test_resident_post_cpu.py, which builds it with AddressSanitizer + UBSan and, for `threads`, a second time with ThreadSanitizer.
//   resident_post_driver layout <n> ...        sizes and offsets of WEntry and Mailbox, then per n the staging slot's size and its four array offsets
//   resident_post_driver post <s>              step s written into an empty mailbox: is its line a whole post of s, s - 8, s + 8; are two lines with one
//                                              stale half each; the payload read back; `posted`; and what is still valid once the ring is forgotten
//   resident_post_driver ledger <op> ...       one PostLedger through a script of transitions, its fields (and the answer of a question) after each:
//                                              select=STEP reselect=STEP deselect restart=STEP absorb=STEP launch=STEP observe=COUNT orphans=POSTED,STEP
//                                              wait=S worker=1|0 hadgpu gaveup clear fallback=MS due=MS      (MS: a time in milliseconds, no clock is read)
//   resident_post_driver stage <n> <steps> <first step> <brake 0|1> <reset 0|1>
//                                              held host-array controls over <steps> steps, staged as resident_post_host does: one line per step
//   resident_post_driver threads <steps>       a writer posts, a reader plays the dispatcher and writes the done flags the writer's ledger waits for
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../triton-racer-sim_amd/csrc/trsim_post.hpp"

using namespace trsim;

static const float* fake(uint64_t s, int which) { return reinterpret_cast<const float*>((uintptr_t)(0x100000u + (s % 100000u) * 64u + (unsigned)which * 4u)); }
static Controls controls_of_step(uint64_t s) { return {fake(s, 0), fake(s, 1), fake(s, 2), reinterpret_cast<const uint8_t*>(fake(s, 3)), (int)(s & 1), 0}; }
static bool payload_is(const WEntry& en, uint64_t s)
{
    const Controls c = controls_of_step(s);
    return en.steer == c.steer && en.thr == c.thr && en.brk == c.brk && en.reset == c.reset && en.synth == (uint32_t)c.synth;
}

static int layout(int argc, char** argv)
{
    std::printf("wentry size=%zu seq_lo=%zu seq=%zu reset=%zu tag_lo=%d tag_hi=%d slots=%d\n", sizeof(WEntry), offsetof(WEntry, seq_lo), offsetof(WEntry, seq),
                offsetof(WEntry, reset), kTagLo, kTagHi, kSlots);
    std::printf("mailbox size=%zu align=%zu close=%zu posted=%zu exited=%zu consumed=%zu error=%zu started=%zu done=%zu ring=%zu\n", sizeof(Mailbox), alignof(Mailbox),
                offsetof(Mailbox, close), offsetof(Mailbox, posted), offsetof(Mailbox, exited), offsetof(Mailbox, consumed), offsetof(Mailbox, error),
                offsetof(Mailbox, started), offsetof(Mailbox, done), offsetof(Mailbox, ring));
    std::printf("codes exit_normal=%llu exit_not_coresident=%llu close_leave=%llu close_cancel=%llu retry_ms0=%u\n", kExitNormal, kExitNotCoresident, kCloseLeave,
                kCloseCancel, kRetryMs0);
    for (unsigned code = 0; code < 12; ++code) std::printf("giveup code=%u text=%s\n", code, give_up_text(code));
    for (int a = 2; a < argc; ++a) {
        const size_t n = (size_t)std::strtoull(argv[a], nullptr, 0);
        std::printf("stage n=%zu slot=%zu steer=%zu thr=%zu brk=%zu reset=%zu\n", n, stage_slot_bytes(n), stage_offset(0, n), stage_offset(1, n), stage_offset(2, n),
                    stage_offset(3, n));
    }
    return 0;
}

static int post(uint64_t s)
{
    Mailbox* mb = new Mailbox();                              // (zeroed; on the heap so that a store beside it is seen)
    write_post(mb, s, controls_of_step(s));
    const WEntry& en = mb->ring[s & (kSlots - 1)];
    WEntry stale_hi = en, stale_lo = en;                     // by hand: a fresh first half beside the second half of step s + 8's post, and the reverse
    stale_hi.seq = s + 8 + 1;
    stale_lo.seq_lo = s + 8 + 1;
    int others = 0;
    for (int k = 0; k < kSlots; ++k) others += (&mb->ring[k] != &en) && (mb->ring[k].seq || mb->ring[k].seq_lo || mb->ring[k].steer);
    std::printf("post s=%" PRIu64 " whole=%d whole_prev=%d whole_next=%d stale_hi=%d stale_hi_next=%d stale_lo=%d stale_lo_next=%d payload=%d posted=%" PRIu64 " others=%d\n", s,
                (int)whole_post(en, s), (int)whole_post(en, s - 8), (int)whole_post(en, s + 8), (int)whole_post(stale_hi, s), (int)whole_post(stale_hi, s + 8),
                (int)whole_post(stale_lo, s), (int)whole_post(stale_lo, s + 8), (int)payload_is(en, s), host_load(&mb->posted), others);
    for (uint64_t t = s + 1; t < s + kSlots; ++t) write_post(mb, t, controls_of_step(t));
    for (int k = 0; k < kSlots; ++k) host_store(&mb->done[k], s + (uint64_t)k + 1);
    int valid_before = 0, valid_after = 0, flags = 0;
    for (uint64_t t = s - 2 * kSlots; t != s + 3 * kSlots; ++t) valid_before += whole_post(mb->ring[t & (kSlots - 1)], t);
    forget_ring(mb);
    for (int k = 0; k < kSlots; ++k)
        for (uint64_t t = s - 2 * kSlots; t != s + 3 * kSlots; ++t) valid_after += t + 1 != 0 && whole_post(mb->ring[k], t);   // (tag 0 is "no post": there is no step 2^64 - 1)
    for (int k = 0; k < kSlots; ++k) flags += host_load(&mb->done[k]) != 0;
    std::printf("forget valid_before=%d valid_after=%d flags=%d posted=%" PRIu64 "\n", valid_before, valid_after, flags, host_load(&mb->posted));
    delete mb;
    return 0;
}

static int ledger(int argc, char** argv)
{
    PostLedger L;
    const PostLedger::Clock::time_point t0{};
    for (int a = 2; a < argc; ++a) {
        const std::string op(argv[a], std::strcspn(argv[a], "="));
        const char* val = argv[a] + op.size() + (argv[a][op.size()] == '=');
        char* rest = nullptr;
        const uint64_t x = std::strtoull(val, &rest, 0), y = *rest == ',' ? std::strtoull(rest + 1, nullptr, 0) : 0;
        const auto at = t0 + std::chrono::milliseconds(x);
        int answer = -1;
        if (op == "select") answer = L.select(x);
        else if (op == "reselect") answer = L.reselect(x);
        else if (op == "deselect") L.deselect();
        else if (op == "restart") L.restart(x);
        else if (op == "absorb") L.absorb(x);
        else if (op == "launch") L.note_launch(x);
        else if (op == "observe") L.observe(x);
        else if (op == "orphans") answer = L.orphans(x, y);
        else if (op == "wait") answer = L.must_wait(x);
        else if (op == "worker") { if (x) L.worker_launched(); else L.worker_ended(); }
        else if (op == "hadgpu") L.worker_had_the_gpu();
        else if (op == "gaveup") L.gave_up();
        else if (op == "clear") L.clear_fault();
        else if (op == "fallback") L.fall_back(at);
        else if (op == "due") answer = L.retry_due(at);
        else { std::fprintf(stderr, "unknown transition: %s\n", argv[a]); return 2; }
        std::printf("%s enabled=%d running=%d launched=%d fell_back=%d broken=%d base=%" PRIu64 " seen_done=%" PRIu64 " retry_ms=%u t_fallback=%lld answer=%d\n", argv[a],
                    (int)L.enabled, (int)L.running, (int)L.launched, (int)L.fell_back, (int)L.broken, L.base, L.seen_done, L.retry_ms,
                    (long long)std::chrono::duration_cast<std::chrono::milliseconds>(L.t_fallback - t0).count(), answer);
    }
    return 0;
}

static int stage(size_t n, int steps, uint64_t first, bool brake, bool reset)
{
    std::vector<float> st(n), th(n), br(n);
    std::vector<uint8_t> rs(n);
    for (size_t i = 0; i < n; ++i) { st[i] = 0.25f * (float)i - 1.0f; th[i] = 100.0f + (float)i; br[i] = -3.0f - (float)i; rs[i] = (uint8_t)(i % 3 == 1); }
    const Controls h{st.data(), th.data(), brake ? br.data() : nullptr, reset ? rs.data() : nullptr, 0, 0};
    std::vector<unsigned char> staging(stage_slot_bytes(n) * kSlots, 0xEE);   // (exactly what ensure_resident allocates: a store past it is caught)
    unsigned char* prev = nullptr;
    for (int k = 0; k < steps; ++k) {
        const uint64_t s = first + (uint64_t)k;
        unsigned char* slot = stage_slot(staging.data(), s, n);
        if (k == 0) stage_fill(slot, h, n); else stage_carry(slot, prev, n);
        stage_carry(slot, slot, n);                          // onto itself: nothing to do (and no overlapping memcpy)
        prev = slot;
        const Controls c = stage_controls(slot, h, n, k == 0);
        const bool floats = !std::memcmp(c.steer, st.data(), n * 4) && !std::memcmp(c.thr, th.data(), n * 4) && (!c.brk || !std::memcmp(c.brk, br.data(), n * 4));
        const bool bytes = !c.reset || !std::memcmp(c.reset, rs.data(), n);
        std::printf("step k=%d slot=%zu steer=%zu thr=%zu brk=%td reset=%td floats=%d bytes=%d synth=%d stride=%d\n", k, (size_t)(slot - staging.data()) / stage_slot_bytes(n),
                    (size_t)(reinterpret_cast<const unsigned char*>(c.steer) - slot), (size_t)(reinterpret_cast<const unsigned char*>(c.thr) - slot),
                    c.brk ? reinterpret_cast<const unsigned char*>(c.brk) - slot : (ptrdiff_t)-1, c.reset ? c.reset - slot : (ptrdiff_t)-1, (int)floats, (int)bytes, c.synth, c.stride);
    }
    return 0;
}

static int threads(uint64_t steps)
{
    Mailbox* mb = new Mailbox();
    uint64_t mismatches = 0, waits = 0;
    std::thread reader([&] {                                 // the dispatcher and the completion flag in one: it sees a post by its SECOND tag, like the device
        for (uint64_t known = 0; known < steps; ++known) {
            const int slot = (int)(known & (kSlots - 1));
            while (host_load(&mb->ring[slot].seq) != known + 1) std::this_thread::yield();
            const WEntry line = mb->ring[slot];
            mismatches += !whole_post(line, known) || !payload_is(line, known);
            host_store(&mb->done[slot], known + 1);
        }
    });
    PostLedger L;
    L.select(0);
    for (uint64_t s = 0; s < steps; ++s) {
        if (L.must_wait(s)) {
            ++waits;
            while (host_load(&mb->done[(s - kSlots) & (kSlots - 1)]) < s - kSlots + 1) std::this_thread::yield();
            L.observe(s - kSlots + 1);
        }
        write_post(mb, s, controls_of_step(s));
    }
    reader.join();
    std::printf("threads steps=%" PRIu64 " mismatches=%" PRIu64 " waits=%" PRIu64 " posted=%" PRIu64 " seen_done=%" PRIu64 "\n", steps, mismatches, waits, host_load(&mb->posted), L.seen_done);
    delete mb;
    return mismatches ? 1 : 0;
}

int main(int argc, char** argv)
{
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "layout") return layout(argc, argv);
    if (cmd == "post" && argc == 3) return post(std::strtoull(argv[2], nullptr, 0));
    if (cmd == "ledger") return ledger(argc, argv);
    if (cmd == "stage" && argc == 7) return stage((size_t)std::atoi(argv[2]), std::atoi(argv[3]), std::strtoull(argv[4], nullptr, 0), std::atoi(argv[5]) != 0, std::atoi(argv[6]) != 0);
    if (cmd == "threads" && argc == 3) return threads(std::strtoull(argv[2], nullptr, 0));
    std::fprintf(stderr, "usage: resident_post_driver layout|post|ledger|stage|threads ... (see the head of tests/resident_post_driver.cpp)\n");
    return 2;
}
