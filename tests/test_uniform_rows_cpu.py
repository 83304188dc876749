"""Uniform rows written once per frame buffer (CPU): the flag transitions of UniformRows and the store-count arithmetic of the resident worker's lagged
arrivals, both from triton-racer-sim_amd/csrc/trsim_plan.hpp through tests/uniform_rows_driver.cpp (host compiler, AddressSanitizer + UBSan)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V_DEPTH, V_DYN, V_HILLS, V_LENS, V_LIGHT = 1, 2, 4, 8, 16


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("uniform") / "driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "uniform_rows_driver.cpp")])
    return str(exe)


def run(driver, *args):
    out = subprocess.run([driver, *[str(a) for a in args]], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    return [line.split(" ") for line in out.stdout.splitlines()]


def flags(driver, *events):
    rows = run(driver, "flags", *events)
    assert [r[1] for r in rows] == list(events)
    return [(int(r[2]), int(r[3]), int(r[4])) for r in rows]


def test_a_buffer_becomes_valid_by_a_plain_step_rendered_into_it(driver):
    # fresh buffers hold nothing; step 6 renders into buffer 0, step 7 into buffer 1; DEPTH and HILLS are plain for this purpose
    assert flags(driver, "invalidate", "render:6:1", "render:7:1") == [(0, 0, 0), (1, 0, 1), (1, 1, 3)]
    assert flags(driver, "render:7:1") == [(0, 1, 2)]
    assert flags(driver, f"variant:{V_DEPTH}", "render:3:1", f"variant:{V_HILLS}", "render:4:1") == [(0, 0, 0), (0, 1, 2), (0, 1, 2), (1, 1, 3)]
    # a launch of several frames (8 steps per launch renders 7 or 8 frames): both buffers; a launch without a frame (r_first > r_last): nothing
    assert flags(driver, "render:11:7") == [(1, 1, 3)]
    assert flags(driver, "render:11:0") == [(0, 0, 0)]


@pytest.mark.parametrize("whole", [V_DYN, V_LENS, V_LIGHT, V_LIGHT | V_DYN, V_LIGHT | V_HILLS, V_LENS | V_DEPTH])
def test_whole_frame_variants_never_skip_and_leave_the_buffer_invalid(driver, whole):
    got = flags(driver, "render:0:2", f"variant:{whole}", "render:2:1", "variant:0", "render:3:1", "render:4:1")
    #                  both valid      mask of the variant: 0    buffer 0 lost     plain again: 1 kept   buffer 1 again   buffer 0 again
    assert got == [(1, 1, 3), (1, 1, 0), (0, 1, 0), (0, 1, 2), (0, 1, 2), (1, 1, 3)]


def test_every_event_that_changes_the_rows_or_the_buffers_clears_both(driver):
    # upload_palette (track load, frame filter, camera, lens, lighting), buffer allocation and a worker that ended by its abort bit all call invalidate()
    assert flags(driver, "render:0:2", "invalidate", "render:5:1", "invalidate") == [(1, 1, 3), (0, 0, 0), (0, 1, 2), (0, 0, 0)]


def test_a_worker_marks_what_it_rendered_at_its_normal_exit(driver):
    # called off (no check-in, cancelled: consumed == start): nothing changes; one step: its buffer; two or more: both
    assert flags(driver, "worker:8:8", "worker:9:10", "worker:12:13", "invalidate", "worker:20:25") == [(0, 0, 0), (0, 1, 2), (1, 1, 3), (0, 0, 0), (1, 1, 3)]
    assert flags(driver, "render:0:2", "worker:4:4") == [(1, 1, 3), (1, 1, 3)]
    # a worker of a whole-frame variant: the buffers it rendered into no longer hold uniform rows
    assert flags(driver, "render:0:2", f"variant:{V_DYN}", "worker:2:3", "variant:0") == [(1, 1, 3), (1, 1, 0), (0, 1, 0), (0, 1, 2)]
    assert flags(driver, "render:0:2", f"variant:{V_LIGHT}", "worker:2:9", "variant:0") == [(1, 1, 3), (1, 1, 0), (0, 0, 0), (0, 0, 0)]


def uni_rows_of(h):
    return (49 * h) // 120          # the default camera on a flat track: 49 of 120 rows


@pytest.mark.parametrize("depth", [0, 1])
@pytest.mark.parametrize("epw", [1, 2, 3, 4])
@pytest.mark.parametrize("h,w", [(60, 80), (120, 160), (240, 320)])
def test_the_counted_wait_never_exceeds_what_the_wave_has_issued(driver, h, w, epw, depth):
    """Every raster wave, every ragged workgroup size up to epw, every host mask, both start parities, four queue patterns, 40 steps of a generation: the
    count of each lagged arrival is at most (here: exactly) the store instructions the wave has issued since the end of the step it arrives for, and each
    step issues worker_step_stores() instructions."""
    n = 0
    for uni in sorted({uni_rows_of(h), 0, 1, h // 2, h}):
        rows = run(driver, "counts", h, w, uni, epw, depth)
        assert len(rows) == 8 * epw * 4 * 2 * 4
        for tag, wave, n_loc, mask, par, pattern, lag, nstep, nuni, waits, worst, wrong in rows:
            assert tag == "counts" and int(wrong) == 0
            assert int(lag) in (2, 3) and int(waits) >= 10
            assert int(worst) <= 0, (uni, wave, n_loc, mask, par, pattern, worst)
            assert int(worst) == 0                                     # exact: a count that were too small would only wait longer, but none is
            steady = int(nstep) - int(nuni)
            assert (int(lag) == 3) == (2 * steady <= 63)
            n += 1
    assert n > 0


def test_flagship_wave_issues_26_instead_of_46_stores_per_step(driver):
    rows = [r for r in run(driver, "counts", 120, 160, 49, 4, 0) if r[1] == "0" and r[2] == "4"]
    assert rows and all((int(r[7]), int(r[8])) == (46, 20) for r in rows)
