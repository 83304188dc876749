"""bench.py prints ONE JSON line with the driver's contract keys (plus, with --full, the roofline / cpu_baseline / also objects), and
--dump-outputs writes what the timed path computed in its last step, the same on every run with the same arguments."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline"}
ROOFLINE = {"bound", "achieved", "peak", "unit", "frac", "traffic"}


@pytest.mark.gpu
def test_bench_line_has_the_contract_keys():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "40", "--warmup", "5", "--envs-per-gpu", "256", "--full"],
                         capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert REQUIRED <= set(d) and ROOFLINE <= set(d["roofline"])
    assert d["n_gpus"] == 1 and d["steps"] == 40 and d["warmup"] == 5 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["unit"] == "env-steps/s" and d["value"] > 1e6 and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    assert d["roofline"]["bound"] == "hbm" and d["roofline"]["peak"] == 8000.0 and 0 < d["roofline"]["frac"] < 1
    cb = d["cpu_baseline"]
    assert {"value", "unit", "cores", "kind", "sample"} <= set(cb) and cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0
    # every BASELINE config has a leg in the driver's line: configs[0] 1 env through the Car loop, configs[1] 256 envs physics only,
    # configs[2] the line itself, configs[3] / [4] one GPU's share
    also = d["also"]
    assert {"config1_car_loop", "physics_256", "shard_512_of_4096", "pilot_closed_loop", "pilot_closed_loop_512x240x320_depth"} <= set(also)
    c1 = also["config1_car_loop"]
    assert "error" not in c1 and c1["ticks_per_s_launch"] > 100 and c1["ticks_per_s_resident"] > 100
    p2 = also["physics_256"]
    assert "error" not in p2 and p2["envs"] == 256 and p2["us_per_step_spl1"] > 0 and p2["us_per_step_spl16"] > 0 and p2["env_steps_per_s_spl16"] > 1e6
    assert p2["tick_launch_us"] > 0 and p2["tick_resident_us"] > 0            # the consumer-paced tick, launched and posted to the resident physics worker
    assert d["value_incl_worker_launch"] > 0 and d["config"]["launcher"] in ("self", "external", "torch.distributed.run")
    # the image path and the filtered step are in the driver's line
    ip = also["image_path"]
    assert "error" not in ip
    for shape in ("1024x120x160", "256x240x320"):
        assert {"trim", "trim_dynamic_brightness", "trim_hsv_masks", "trim_dynamic_masks_canny"} <= set(ip[shape])
        for leg in ip[shape].values():
            assert leg["us_per_batch"] > 0 and leg["GBps"] > 0 and 0 < leg["frac_of_hbm_peak"] < 1
    fs = also["filtered_step"]
    assert "error" not in fs and {"raw_frames", "static_palette_filter", "dynamic_brightness"} <= set(fs)
    assert all(fs[k]["us_per_step"] > 0 for k in ("raw_frames", "static_palette_filter", "dynamic_brightness"))
    ht = also["hilly_track"]                                                 # a track with elevation (round 5): the mountain track's step in the driver's line
    assert "error" not in ht and ht["rgb"]["us_per_step"] > 0 and ht["rgb_depth"]["us_per_step"] > 0 and 0 < ht["rgb"]["frac_of_hbm_peak"] < 1


def _json_lines(out):
    return [l for l in out.stdout.splitlines() if l.strip().startswith("{")]


def _load_dump(d):
    files = sorted(os.listdir(d))
    assert files and all(f.endswith(".npy") for f in files), files
    assert sum(os.path.getsize(os.path.join(d, f)) for f in files) <= 64 << 20
    out = {f[:-4]: np.load(os.path.join(d, f)) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values()), {k: a.dtype.name for k, a in out.items()}
    return out


@pytest.mark.gpu
def test_plain_bench_line_is_lean_and_its_outputs_reproduce(tmp_path):
    """A plain run: the headline keys, none of the --full extras, exactly --steps timed steps; --dump-outputs twice with the same arguments
    gives the same arrays (the pre-warm is a fixed number of steps, the synthetic controls are keyed by the step count)."""
    dumps = []
    for tag in ("a", "b"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "40", "--warmup", "5", "--envs-per-gpu", "256",
                              "--dump-outputs", str(tmp_path / tag)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = _json_lines(out)
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"} <= set(d)
        assert not {"roofline", "also", "cpu_baseline", "value_incl_worker_launch"} & set(d)       # resident mode: the roofline takes a pass of its own
        assert d["steps"] == 40 and d["warmup"] == 5 and d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["value"] > 1e6
        assert abs(d["ms_per_step"] - 256 * 40 / d["value"] / 40 * 1e3) <= 1e-3 * d["ms_per_step"] + 1e-6
        dumps.append(_load_dump(tmp_path / tag))
    a, b = dumps
    assert set(a) == set(b) and {"pos_x", "speed", "cte", "seg_idx", "done", "img", "img_env_idx"} <= set(a)
    assert a["pos_x"].shape == (256,) and a["img"].shape[1:] == (120, 160, 3) and a["img"].shape[0] == a["img_env_idx"].shape[0]
    assert a["img"].max() > 0
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_dump_outputs_sizes_and_types(oracle_api, tmp_path, monkeypatch):
    """bench.dump_outputs on the CPU oracle's env: float32 / float64 files only, frames of a seeded sample of the envs, the per-env values of a
    seeded sample too once they outgrow their budget; the same env state gives the same files."""
    import bench
    from triton_racer_sim_amd.env import BatchedEnv
    env = BatchedEnv(n_envs=40, auto_reset=True, depth=True, _api=oracle_api)
    env.step_synthetic(12, 1)
    monkeypatch.setattr(bench, "DUMP_FRAME_BYTES", 5 * 120 * 160 * 4 * 4)
    bench.dump_outputs(env, str(tmp_path / "a"))
    a = _load_dump(tmp_path / "a")
    assert a["img"].shape == (5, 120, 160, 3) and a["depth"].shape == (5, 120, 160) and "env_idx" not in a
    idx = a["img_env_idx"].astype(int)
    assert np.array_equal(a["img"], env.fetch("img")[idx].astype(np.float32)) and np.array_equal(a["pos_x"], env.fetch("pos_x"))
    assert np.array_equal(a["seg_idx"], env.fetch("seg_idx").astype(np.float64))
    monkeypatch.setattr(bench, "DUMP_ENV_BYTES", 10 * (4 * 8 + 8 * 3))
    bench.dump_outputs(env, str(tmp_path / "b"))
    b = _load_dump(tmp_path / "b")
    sel = b["env_idx"].astype(int)
    assert sel.shape == (10,) and np.array_equal(b["speed"], env.fetch("speed")[sel]) and np.array_equal(b["img"], a["img"])
    env.close()


def test_prewarm_is_a_fixed_step_count():
    """The untimed pre-warm is a number of steps fixed by the arguments (about PREWARM_S of work: ~8,400 steps of the default workload)."""
    import bench
    chunks, chunk = bench.prewarm_steps(1024, 120, 160, True, False)
    assert (chunks, chunk) == bench.prewarm_steps(1024, 120, 160, True, False) and 7000 <= chunks * chunk <= 10000
    _, macs = bench.pilot_weights(120, 160)
    chunks, chunk = bench.prewarm_steps(1024, 120, 160, True, False, 2.0 * macs)
    assert chunk == 50 and 300 <= chunks * chunk <= 700


@pytest.mark.gpu
def test_bench_self_launch_on_the_gpu():
    """`python bench.py --gpus 1 --spawn`: the rank runs as a child of a parent that never touches the GPU — the path `--gpus N` takes for N > 1."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--spawn", "--steps", "40", "--warmup", "5", "--envs-per-gpu", "256",
                          "--no-also", "--no-cpu-baseline"], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = _json_lines(out)
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["config"]["launcher"] == "self" and d["value"] > 1e6 and "allgather" not in d


@pytest.mark.gpu
def test_bench_two_ranks_rehearsal_sharing_the_gpu():
    """The N > 1 branch of bench.py end to end on the one GPU of this box: two self-launched ranks, each with its own shard, K steps between host
    barriers, MAX over ranks, one all-gather timed on its own.  Both ranks share GPU 0, so the group is gloo (RCCL refuses two ranks on one device)
    and the value is not a measurement — the line says so.  Both ranks select RESIDENT mode, as the real run does: the library lets one worker at a
    time have the GPU (round 5: a launch that does not get the whole GPU is called off and that rank steps by launches until its next try; round 4
    failed here with "resident worker gave up", gpurun_out/r04_full_2.log, and had to rehearse with launches)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-gpu", "--steps", "20", "--warmup", "5", "--total-envs", "512"],
                         capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = _json_lines(out)
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 20 and d["config"]["envs_total"] == 512 and d["config"]["envs_per_gpu"] == 256
    assert d["config"]["launcher"] == "self" and "rehearsal" in d["config"]
    ag = d["allgather"]
    assert ag["ranks"] == 2 and ag["floats_per_rank"] == 256 and ag["us"] > 0 and ag["backend"] == "gloo"
    assert d["value"] > 0 and d["ms_per_step"] > 0 and "cpu_baseline" not in d
    assert ag["values"] == 512 and "unmeasured on hardware" in d["config"]["n_gt_1_status"]
    assert d["config"]["step_mode"].startswith("resident") and d["config"]["step_mode_at_end"]["mode"] in ("resident", "launch")


@pytest.mark.gpu
def test_bench_nccl_branch_at_world_size_one():
    """`--force-dist`: the process groups of the N > 1 branch at world size 1 on this box's GPU — nccl (= RCCL) for the one all-gather, a gloo group
    for the host barriers and the MAX over ranks — and the exchange through nccl: every call of the N > 1 branch that the two-rank rehearsal (gloo
    only: RCCL refuses two ranks on one device) cannot reach."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--force-dist", "--steps", "20", "--warmup", "5", "--envs-per-gpu", "512",
                          "--no-also", "--no-cpu-baseline"], capture_output=True, text=True, timeout=900, cwd=ROOT,
                         env=dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29571"))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = _json_lines(out)
    assert len(lines) == 1
    d = json.loads(lines[0])
    ag = d["allgather"]
    assert ag["backend"] == "nccl" and ag["ranks"] == 1 and ag["floats_per_rank"] == 512 and ag["us"] > 0
    assert d["n_gpus"] == 1 and d["value"] > 1e6
