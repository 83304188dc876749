"""The tick loop of the closed loops without a GPU (trs_step_pilot, trs_step_expert, trs_step_dagger): triton-racer-sim_amd/csrc/trsim_loop.hpp, the header
alone, through tests/loop_driver.cpp (host compiler, AddressSanitizer + UBSan) — the real ``closed_loop`` over scripted ops, every case in ONE child process —
against a Python statement of the order of a tick.  The slot rule is ``capture_plan`` of tests/test_expert_cpu.py.  What a call leaves behind when an op
fails half-way (the counter, ``*n_captured``, which ops went out) can only be tested here: on the device no failure is provoked."""
import itertools
import os
import shutil
import subprocess

import pytest

from test_expert_cpu import capture_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ("observe", "label", "keep", "step")
CODE = -3                                                    # what an injected failure returns

# (n_steps, every, skip, capacity, capture, first tick with a frame, k at the start or None, failure (tick, op) or None)
PLAIN = [(n, every, skip, capacity, capture, first, k0, None)
         for n, every, skip, capacity, capture, first, k0 in itertools.product((1, 3, 5), (1, 2), (0, 1), (0, 2, 100), ("rows", "frames"), (0, 1), (0, 7, None))]
PLAIN += [(n, 1, 0, 100, "none", first, k0, None) for n in (1, 3) for first in (0, 1) for k0 in (0, 7, None)]      # (none, None): trs_step_pilot's form
FAILING = [(3, 1, 0, capacity, capture, 0, k0, (1, op)) for op in OPS for capture in ("rows", "frames") for capacity in (1, 100) for k0 in (0, 7, None)]
CASES = PLAIN + FAILING


def tick_order(n_steps, every, skip, capacity, capture, first_frame, k0, fail):
    """The statement: (lines, return code, *n_captured, k) of one call."""
    wants_frames, counted = capture == "frames", k0 is not None
    slots = [-1] * n_steps
    if capture != "none" and counted:
        # a call of k0 ticks brings the counter to k0; the call under test follows it, with a frame from its tick first_frame on (when no frame is wanted: always)
        ticks, _ = capture_plan(every, skip, capacity, k0 + first_frame if wants_frames else 0, [k0, n_steps])[1]
        assert [k for k, _ in ticks] == list(range(k0, k0 + n_steps))
        slots = [s for _, s in ticks]
    lines, k, n_captured = [], k0, 0

    def issue(t, op, text):
        lines.append(f"tick {t} {text}")
        return fail == (t, op)

    for t in range(n_steps):
        if issue(t, "observe", "observe"):
            return lines, CODE, n_captured, k
        if issue(t, "label", f"label slot {slots[t]}"):
            return lines, CODE, n_captured, k
        if counted:
            k += 1
        if slots[t] >= 0 and wants_frames and issue(t, "keep", f"keep slot {slots[t]}"):
            return lines, CODE, n_captured, k
        n_captured = sum(s >= 0 for s in slots[:t + 1])
        if issue(t, "step", "step"):
            return lines, CODE, n_captured, k
    return lines, 0, n_captured, k


def argv_of(case):
    n, every, skip, capacity, capture, first, k0, fail = case
    return [n, every, skip, capacity, capture, first, "none" if k0 is None else k0] + ([fail[0], fail[1], CODE] if fail else [])


@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    """What the driver printed per case: (lines, return code, *n_captured, k)."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("loop") / "driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "loop_driver.cpp")])
    args = []
    for case in CASES:
        args += ["--"] * bool(args) + [str(a) for a in argv_of(case)]
    out = subprocess.run([str(exe), *args], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    got = []
    for line in out.stdout.splitlines():
        if line.startswith("case "):
            assert int(line.split()[1]) == len(got)
            got.append([])
        else:
            got[-1].append(line)
    assert len(got) == len(CASES)
    tail = lambda block: (block[:-3], int(block[-3].split()[1]), int(block[-2].split()[1]), None if block[-1] == "k none" else int(block[-1].split()[1]))
    for block in got:
        assert [l.split()[0] for l in block[-3:]] == ["rc", "n_captured", "k"], block
    return dict(zip(CASES, map(tail, got)))


@pytest.mark.parametrize("case", PLAIN, ids=lambda c: "-".join(str(a) for a in c[:7]))
def test_a_call_issues_the_ops_in_the_stated_order(traces, case):
    n_steps, every, skip, capacity, capture, first_frame, k0, _ = case
    lines, rc, n_captured, k = traces[case]
    assert (lines, rc, n_captured, k) == tick_order(*case)
    assert rc == 0 and k == (None if k0 is None else k0 + n_steps)
    assert [l for l in lines if l.endswith(" observe") or l.endswith(" step")] == [f"tick {t} {op}" for t in range(n_steps) for op in ("observe", "step")]   # every tick observes and steps
    slots = [int(l.split()[-1]) for l in lines if " label slot " in l]
    assert len(slots) == n_steps                             # every tick labels, captured or not
    assert [s for s in slots if s >= 0] == list(range(n_captured)) and n_captured <= capacity
    kept = [int(l.split()[-1]) for l in lines if " keep slot " in l]
    assert kept == ([s for s in slots if s >= 0] if capture == "frames" else [])
    if capture == "frames" and first_frame == 1:
        assert slots[0] == -1                                # a tick with no frame takes no slot
    if k0 is None or capture == "none":
        assert n_captured == 0 and not kept and all(s == -1 for s in slots)     # no counter, or no capture: nothing is captured


def test_the_cases_capture_something(traces):
    """The plain cases are not vacuous: some fill their capacity, some are cut short by it, some skip the frameless first tick and capture the next."""
    used = {case: traces[case][2] for case in PLAIN}
    assert any(u == 2 and c[3] == 2 and c[0] == 5 for c, u in used.items()) and any(u == 5 for u in used.values())
    assert any(traces[c][0][:5] == ["tick 0 observe", "tick 0 label slot -1", "tick 0 step", "tick 1 observe", "tick 1 label slot 0"] for c in PLAIN if c[4] == "frames" and c[5] == 1)


@pytest.mark.parametrize("case", FAILING, ids=lambda c: "-".join(str(a) for a in c[3:7]) + "-" + c[7][1])
def test_a_failed_op_ends_the_call_where_it_stands(traces, case):
    _, _, _, capacity, capture, _, k0, (tick, op) = case
    lines, rc, n_captured, k = traces[case]
    assert (lines, rc, n_captured, k) == tick_order(*case)
    captured = k0 is not None                                # every = 1, skip = 0, a frame from tick 0 on: a driver's tick is captured while slots are left
    keeps = capture == "frames" and captured and capacity > tick
    if op == "keep" and not keeps:                           # the op is not issued at that tick: nothing fails
        assert rc == 0 and len([l for l in lines if l.endswith(" step")]) == 3
        return
    assert rc == CODE
    assert lines[-1].startswith(f"tick {tick} {op}")         # nothing is issued after the failing op
    assert not any(l.startswith(f"tick {tick + 1} ") for l in lines)
    if k0 is not None:
        assert k == k0 + tick + (op in ("keep", "step"))     # the counter has moved iff the label went out
    # *n_captured is what the last completed update left: tick 0's, or tick 1's when the failure came behind it (the step)
    done = tick + (op == "step")
    assert n_captured == (min(done, capacity) if captured else 0)
