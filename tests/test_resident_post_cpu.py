"""The host's half of the resident worker's post protocol (csrc/trsim_post.hpp) on the CPU: tests/resident_post_driver.cpp built with AddressSanitizer + UBSan
and run as a subprocess, its two-thread case a second time with ThreadSanitizer.  The expected values are those of the host code as it stood in
trsim_resident.hip before the header existed — `base = seen_done = step_count` at every restart, a slot wait from `s >= base + 8` on, the orphan test
`posted > seen_done && posted == step_count`, a retry interval of 100 ms doubling up to 2 s — written out here, not read back from the header."""
import os
import platform
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZERS = {"asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "tsan": ["-fsanitize=thread", "-pthread"]}


def build_driver(directory, kind):
    if not shutil.which("g++"):
        return None
    exe = os.path.join(str(directory), "resident_post_driver_" + kind)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + SANITIZERS[kind] + ["-o", exe, os.path.join(ROOT, "tests", "resident_post_driver.cpp")])
    return exe


def run_driver(exe, *args, prefix=()):
    out = subprocess.run(list(prefix) + [exe] + [str(a) for a in args], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=60)
    assert out.returncode == 0, (args, out.stdout[-500:], out.stderr[-2000:])
    assert not re.search(r"runtime error|AddressSanitizer|ThreadSanitizer", out.stderr), out.stderr[-2000:]
    return [parse(line) for line in out.stdout.splitlines()]


def parse(line):
    """'kind a=1 b=x text=the rest' -> (kind, {a: 1, b: 'x', text: 'the rest'})"""
    kind, _, rest = line.partition(" ")
    rest, sep, text = rest.partition("text=")
    rec = {k: (int(v) if re.fullmatch(r"-?\d+", v) else v) for k, v in (kv.split("=", 1) for kv in rest.split())}
    if sep:
        rec["text"] = text
    return kind, rec


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = build_driver(tmp_path_factory.mktemp("resident_post"), "asan")
    if not exe:
        pytest.skip("g++ not available")
    return exe


# ---- 1. layout -----------------------------------------------------------------------------------------------------------------------------

def test_layout_of_the_mailbox_and_the_staging_slot(driver):
    sizes = (1, 5, 64, 1024)
    lines = run_driver(driver, "layout", *sizes)
    wentry, mailbox, codes = lines[0][1], lines[1][1], lines[2][1]
    assert wentry == {"size": 64, "seq_lo": 0, "seq": 48, "reset": 32, "tag_lo": 0, "tag_hi": 6, "slots": 8}     # the tags are u64 words 0 and 6 of the line
    assert (mailbox["close"], mailbox["posted"], mailbox["exited"], mailbox["consumed"], mailbox["error"], mailbox["started"]) == (0, 8, 64, 72, 80, 88)
    assert (mailbox["done"], mailbox["ring"], mailbox["size"], mailbox["align"]) == (128, 192, 192 + 8 * 64, 64)
    for field in ("close", "exited", "done", "ring"):                          # each starts a 64-byte line: what the device reads or writes alone
        assert mailbox[field] % 64 == 0, field
    assert codes == {"exit_normal": 1, "exit_not_coresident": 2, "close_leave": 1, "close_cancel": 2, "retry_ms0": 100}
    texts = {rec["code"]: rec["text"] for kind, rec in lines if kind == "giveup"}
    assert texts == {0: "", 1: "waiting for a post", 2: "camera ring back-pressure", 3: "waiting for the physics team", 4: "forwarding the last arrivals",
                     5: "team barrier of the dynamic-brightness batch", 6: "", 7: "abort injected by trs_resident_debug_abort (test hook)", 8: "",
                     9: "dynamic LDS segment not at offset 0", 10: "?", 11: "?"}
    stages = [rec for kind, rec in lines if kind == "stage"]
    assert [r["n"] for r in stages] == list(sizes)
    for r in stages:
        n = r["n"]
        assert r["slot"] == (13 * n + 63) & ~63 and (r["steer"], r["thr"], r["brk"], r["reset"]) == (0, 4 * n, 8 * n, 12 * n)


# ---- 2. the post ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", [0, 7, 8, 2 ** 32 + 3])
def test_a_post_is_whole_for_its_step_alone(driver, s):
    (_, post), (_, forget) = run_driver(driver, "post", s)
    assert post["s"] == s and post["whole"] == 1 and (post["whole_prev"], post["whole_next"]) == (0, 0)
    assert (post["stale_hi"], post["stale_hi_next"], post["stale_lo"], post["stale_lo_next"]) == (0, 0, 0, 0)     # halves of different posts never pair
    assert post["payload"] == 1 and post["posted"] == s + 1 and post["others"] == 0
    assert forget == {"valid_before": 8, "valid_after": 0, "flags": 0, "posted": s + 8}        # 8 posts in the ring, none once it is forgotten; `posted` is the host's own


# ---- 3. ledger scripts ---------------------------------------------------------------------------------------------------------------------

FIELDS = ("enabled", "running", "launched", "fell_back", "broken", "base", "seen_done", "retry_ms", "answer")


def run_script(exe, script):
    """script: [(transition, (enabled, running, launched, fell_back, broken, base, seen_done, retry_ms, answer)), ...]; answer -1 = the transition asks nothing"""
    lines = run_driver(exe, "ledger", *[op for op, _ in script])
    assert len(lines) == len(script)
    for i, ((op, want), (kind, rec)) in enumerate(zip(script, lines)):
        assert kind == op and tuple(rec[f] for f in FIELDS) == tuple(want), (i, op, dict(zip(FIELDS, want)), rec)
    return [rec for _, rec in lines]


@pytest.mark.parametrize("step", [0, 41])
def test_ledger_selecting_resident_mode(driver, step):
    run_script(driver, [(f"select={step}", (1, 0, 0, 0, 0, step, step, 100, 1)),          # was off: the ledger starts at the step counter, `posted` must follow
                        (f"select={step + 5}", (1, 0, 0, 0, 0, step, step, 100, 0)),      # selected already: nothing restarts
                        ("deselect", (0, 0, 0, 0, 0, step, step, 100, -1)),
                        (f"select={step + 9}", (1, 0, 0, 0, 0, step + 9, step + 9, 100, 1))])


@pytest.mark.parametrize("start", [0, 41])
def test_ledger_slot_waits_begin_at_the_ninth_step_in_flight(driver, start):
    script = [(f"select={start}", (1, 0, 0, 0, 0, start, start, 100, 1)), ("worker=1", (1, 1, 0, 0, 0, start, start, 100, -1))]
    seen = start
    for s in range(start, start + 20):
        must = s >= start + 8                                                  # eight posts fit the ring; the ninth needs the slot of the first
        script.append((f"wait={s}", (1, 1, 0, 0, 0, start, seen, 100, int(must))))
        if must:
            seen = s - 8 + 1                                                   # wait_done(s - 8) saw done[(s - 8) % 8] == s - 7, late: only when asked for
            script.append((f"observe={seen}", (1, 1, 0, 0, 0, start, seen, 100, -1)))
    recs = run_script(driver, script)
    waits = [r["answer"] for r in recs if r["answer"] >= 0][1:]
    assert waits == [0] * 8 + [1] * 12
    # a flag or a count that is behind what has been seen changes nothing
    run_script(driver, [("select=41", (1, 0, 0, 0, 0, 41, 41, 100, 1)), ("observe=50", (1, 0, 0, 0, 0, 41, 50, 100, -1)), ("observe=44", (1, 0, 0, 0, 0, 41, 50, 100, -1)),
                        ("observe=50", (1, 0, 0, 0, 0, 41, 50, 100, -1))])


def test_ledger_posts_an_eviction_left_in_the_ring(driver):
    run_script(driver, [("select=0", (1, 0, 0, 0, 0, 0, 0, 100, 1)), ("worker=1", (1, 1, 0, 0, 0, 0, 0, 100, -1)),
                        # 10 steps posted, the evicted worker consumed 7 and left: steps 7, 8, 9 stay in the ring
                        ("worker=0", (1, 0, 0, 0, 0, 0, 0, 100, -1)), ("observe=7", (1, 0, 0, 0, 0, 0, 7, 100, -1)),
                        ("orphans=10,10", (1, 0, 0, 0, 0, 0, 7, 100, 1)),                  # the step counter is where the posts end: they are served by the next worker
                        ("orphans=10,11", (1, 0, 0, 0, 0, 0, 7, 100, 0)),                  # a launched step has moved the counter: the ring is of the past
                        ("orphans=10,0", (1, 0, 0, 0, 0, 0, 7, 100, 0)),                   # ... or the counter restarted
                        ("observe=10", (1, 0, 0, 0, 0, 0, 10, 100, -1)),
                        ("orphans=10,10", (1, 0, 0, 0, 0, 0, 10, 100, 0))])               # everything posted is done: nothing is left behind


def test_ledger_fall_back_and_retry_interval(driver):
    script = [("select=0", (1, 0, 0, 0, 0, 0, 0, 100, 1)), ("worker=1", (1, 1, 0, 0, 0, 0, 0, 100, -1)),
              # 12 posted, 7 consumed when the launch is found not co-resident: five posts are replayed as launches
              ("worker=0", (1, 0, 0, 0, 0, 0, 0, 100, -1)), ("fallback=1000", (0, 0, 0, 1, 0, 0, 0, 100, -1)), ("observe=7", (0, 0, 0, 1, 0, 0, 7, 100, -1)),
              ("launch=12", (0, 0, 1, 1, 0, 12, 12, 100, -1)),
              ("due=1000", (0, 0, 1, 1, 0, 12, 12, 100, 0)), ("due=1099", (0, 0, 1, 1, 0, 12, 12, 100, 0)), ("due=1100", (0, 0, 1, 1, 0, 12, 12, 100, 1)),
              ("reselect=15", (1, 0, 0, 0, 0, 15, 15, 200, 1)), ("due=9999", (1, 0, 0, 0, 0, 15, 15, 200, 0))]      # selected again: nothing is due
    now, step = 2000, 15
    for interval in (200, 400, 800, 1600, 2000, 2000):                         # the GPU stays shared: every retry falls back again
        script += [(f"fallback={now}", (0, 0, 0, 1, 0, step, step, interval, -1)),
                   (f"due={now + interval - 1}", (0, 0, 0, 1, 0, step, step, interval, 0)), (f"due={now + interval}", (0, 0, 0, 1, 0, step, step, interval, 1)),
                   (f"reselect={step + 1}", (1, 0, 0, 0, 0, step + 1, step + 1, min(2 * interval, 2000), 1))]
        now, step = now + interval, step + 1
    script += [("hadgpu", (1, 0, 0, 0, 0, step, step, 100, -1))]                # a launch reported in: the sharing is over
    run_script(driver, script)
    # the caller selects resident mode itself while the handle is in its fall-back: the interval starts over, the launched steps stay to be waited for
    run_script(driver, [("select=0", (1, 0, 0, 0, 0, 0, 0, 100, 1)), ("fallback=10", (0, 0, 0, 1, 0, 0, 0, 100, -1)), ("launch=3", (0, 0, 1, 1, 0, 3, 3, 100, -1)),
                        ("due=110", (0, 0, 1, 1, 0, 3, 3, 100, 1)), ("reselect=3", (1, 0, 0, 0, 0, 3, 3, 200, 1)), ("fallback=200", (0, 0, 0, 1, 0, 3, 3, 200, -1)),
                        ("launch=4", (0, 0, 1, 1, 0, 4, 4, 200, -1)), ("select=4", (1, 0, 1, 0, 0, 4, 4, 100, 1))])


def test_ledger_broken_survives_everything_but_a_clear(driver):
    script = [("select=3", (1, 0, 0, 0, 0, 3, 3, 100, 1)), ("worker=1", (1, 1, 0, 0, 0, 3, 3, 100, -1)), ("worker=0", (1, 0, 0, 0, 0, 3, 3, 100, -1)),
              ("gaveup", (1, 0, 0, 0, 1, 3, 3, 100, -1)), ("restart=9", (1, 0, 0, 0, 1, 9, 9, 100, -1)), ("absorb=9", (1, 0, 0, 0, 1, 9, 9, 100, -1)),
              ("launch=10", (1, 0, 1, 0, 1, 10, 10, 100, -1)), ("observe=12", (1, 0, 1, 0, 1, 10, 12, 100, -1)), ("deselect", (0, 0, 1, 0, 1, 10, 12, 100, -1)),
              ("select=12", (1, 0, 1, 0, 1, 12, 12, 100, 1)), ("fallback=50", (0, 0, 1, 1, 1, 12, 12, 100, -1)),
              ("due=5000", (0, 0, 1, 1, 1, 12, 12, 100, 0)),                   # no retry on a handle whose env state is undefined
              ("hadgpu", (0, 0, 1, 1, 1, 12, 12, 100, -1)), ("clear", (0, 0, 1, 1, 0, 12, 12, 100, -1)), ("due=5000", (0, 0, 1, 1, 0, 12, 12, 100, 1))]
    run_script(driver, script)


def test_ledger_a_launched_step_then_absorb(driver):
    run_script(driver, [("select=20", (1, 0, 0, 0, 0, 20, 20, 100, 1)),
                        ("launch=21", (1, 0, 1, 0, 0, 21, 21, 100, -1)),       # trs_step_pilot in resident mode: no post, no flag
                        ("restart=21", (1, 0, 1, 0, 0, 21, 21, 100, -1)),      # a quiesce restarts the ledger and leaves the launched step to be waited for
                        ("wait=28", (1, 0, 1, 0, 0, 21, 21, 100, 0)), ("wait=29", (1, 0, 1, 0, 0, 21, 21, 100, 1)),
                        ("absorb=21", (1, 0, 0, 0, 0, 21, 21, 100, -1)),       # the stream has been waited for (or the next post's worker runs behind the launch)
                        ("launch=22", (1, 0, 1, 0, 0, 22, 22, 100, -1)), ("launch=23", (1, 0, 1, 0, 0, 23, 23, 100, -1)), ("absorb=23", (1, 0, 0, 0, 0, 23, 23, 100, -1))])


def test_ledger_the_step_counter_restarts_below_the_ledger(driver):
    run_script(driver, [("select=0", (1, 0, 0, 0, 0, 0, 0, 100, 1)), ("observe=41", (1, 0, 0, 0, 0, 0, 41, 100, -1)), ("restart=41", (1, 0, 0, 0, 0, 41, 41, 100, -1)),
                        # the track is loaded again: step_count = 0, `posted` still 41
                        ("orphans=41,0", (1, 0, 0, 0, 0, 41, 41, 100, 0)), ("wait=0", (1, 0, 0, 0, 0, 41, 41, 100, 0)),
                        ("absorb=0", (1, 0, 0, 0, 0, 0, 0, 100, -1)),          # the first post without a worker starts the ledger at the counter
                        ("observe=0", (1, 0, 0, 0, 0, 0, 0, 100, -1)),
                        ("wait=7", (1, 0, 0, 0, 0, 0, 0, 100, 0)), ("wait=8", (1, 0, 0, 0, 0, 0, 0, 100, 1))])


# ---- 4. staging ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("brake,reset", [(1, 1), (0, 0), (1, 0), (0, 1)])
def test_staging_of_held_controls_over_more_steps_than_slots(driver, brake, reset):
    n, steps, first = 5, 19, 3
    lines = run_driver(driver, "stage", n, steps, first, brake, reset)
    assert len(lines) == steps
    for k, (kind, r) in enumerate(lines):
        assert kind == "step" and r["k"] == k and r["slot"] == (first + k) % 8, r          # the slot of the step that reads it
        assert (r["steer"], r["thr"]) == (0, 4 * n) and r["brk"] == (8 * n if brake else -1), r
        assert r["reset"] == (12 * n if reset and k == 0 else -1), r                          # the reset mask belongs to the call's first step alone
        assert (r["floats"], r["bytes"], r["synth"], r["stride"]) == (1, 1, 0, 0), r


# ---- 5. two threads ------------------------------------------------------------------------------------------------------------------------

THREADS = {"steps": 2000, "mismatches": 0, "waits": 1992, "posted": 2000, "seen_done": 1992}      # every step from the ninth on waits for the flag of the step 8 before it


def without_address_randomisation():
    """ThreadSanitizer's runtime of g++ 11 refuses to start ("unexpected memory mapping") where the kernel randomises mappings over more bits than its shadow
    layout expects (vm.mmap_rnd_bits above 28): its driver, that one process, runs with the randomisation off where setarch can do that."""
    setarch = shutil.which("setarch")
    prefix = [setarch, platform.machine(), "-R"] if setarch else []
    return prefix if prefix and subprocess.run(prefix + ["true"], capture_output=True).returncode == 0 else []


def test_writer_and_dispatcher_threads_under_tsan(tmp_path):
    exe = build_driver(tmp_path, "tsan")
    if not exe:
        pytest.skip("g++ not available")
    assert run_driver(exe, "threads", 2000, prefix=without_address_randomisation()) == [("threads", THREADS)]


def test_writer_and_dispatcher_threads_under_asan(driver):
    assert run_driver(driver, "threads", 2000) == [("threads", THREADS)]
