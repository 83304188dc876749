// Test driver (CPU): the tick loop of the closed loops (triton-racer-sim_amd/csrc/trsim_loop.hpp — the header alone) run over scripted ops and printed for
// tests/test_loop_cpu.py, which builds it with AddressSanitizer + UBSan and compares the trace with a Python statement of the tick order.
//   loop_driver <case> [-- <case> ...]      one call of closed_loop per case, "case <i>" in front of its lines
//   case: <n_steps> <every> <skip> <capacity> <capture: none | rows | frames> <first tick with a frame> <k at the start | none>
//         [<tick> <observe | label | keep | step> <code>]          the op of that tick returns <code> instead of 0
// Per case one line per op issued: "tick <t> observe", "tick <t> label slot <s>", "tick <t> keep slot <s>", "tick <t> step"; then "rc <code>",
// "n_captured <slots>" and "k <counter | none>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../triton-racer-sim_amd/csrc/trsim_loop.hpp"

namespace {

struct ScriptedOps {
    std::vector<uint8_t> frames;        // one byte per tick stands for that tick's frame
    int first_frame, fail_tick; const char* fail_op; int fail_code;
    int t;                              // the tick in flight: observe opens it
    int result(const char* op) const { return t == fail_tick && !std::strcmp(op, fail_op) ? fail_code : 0; }
    int observe(const uint8_t** frame)
    {
        ++t;
        std::printf("tick %d observe\n", t);
        *frame = t >= first_frame ? &frames[(size_t)t] : nullptr;
        return result("observe");
    }
    int label(int slot)
    {
        std::printf("tick %d label slot %d\n", t, slot);
        return result("label");
    }
    int keep_frame(int slot, const uint8_t* frame)
    {
        std::printf("tick %d keep slot %d%s\n", t, slot, frame == &frames[(size_t)t] ? "" : " of another tick's frame");
        return result("keep");
    }
    int step()
    {
        std::printf("tick %d step\n", t);
        return result("step");
    }
};

int run_case(int argc, char** argv)   // argv[0]: the case's first argument
{
    if (argc != 7 && argc != 10) return 2;
    const int n_steps = std::atoi(argv[0]);
    static float rows[8];
    static uint8_t frames[8];
    trs_expert_capture c{};
    c.struct_size = sizeof c;
    c.every = std::atoi(argv[1]); c.skip = std::atoi(argv[2]); c.capacity = std::atoi(argv[3]); c.d_rows = rows;
    const bool none = !std::strcmp(argv[4], "none");
    if (!std::strcmp(argv[4], "frames")) c.d_frames_or_null = frames;
    else if (!none && std::strcmp(argv[4], "rows")) return 2;
    if (trsim::expert_capture_error(&c, true) || n_steps < 1) return 2;
    const bool counted = std::strcmp(argv[6], "none") != 0;
    uint32_t k = counted ? (uint32_t)std::strtoul(argv[6], nullptr, 10) : 0;
    const bool fails = argc == 10;
    ScriptedOps ops{std::vector<uint8_t>((size_t)n_steps), std::atoi(argv[5]), fails ? std::atoi(argv[7]) : -1, fails ? argv[8] : "", fails ? std::atoi(argv[9]) : 0, -1};
    int n_captured = -1;
    const int rc = trsim::closed_loop(ops, n_steps, none ? nullptr : &c, counted ? &k : nullptr, &n_captured);
    std::printf("rc %d\nn_captured %d\n", rc, n_captured);
    if (counted) std::printf("k %u\n", k);
    else std::printf("k none\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    int cases = 0;
    for (int a = 1; a < argc;) {
        int b = a;
        while (b < argc && std::strcmp(argv[b], "--")) ++b;
        std::printf("case %d\n", cases++);
        if (int rc = run_case(b - a, argv + a)) return rc;
        a = b + 1;
    }
    return cases ? 0 : 2;
}
