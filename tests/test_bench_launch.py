"""bench.py's start-up contract: `python bench.py --gpus N` must start as the driver calls it -- no launcher, no
RANK / WORLD_SIZE -- and a run that cannot start prints ONE JSON line carrying "error", never a traceback.  (The run itself is
rehearsed on a GPU in tests/test_gpu_multi_device.py::test_c4_rehearsal_three_ranks_full_batch_on_one_gpu.)"""
import json
import os
import subprocess
import sys

from conftest import ROOT

CLEAN = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}


def _one_line(proc):
    lines = [ln for ln in proc.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, (proc.stdout[-500:], proc.stderr[-1500:])
    assert "Traceback" not in proc.stderr, proc.stderr[-1500:]
    return json.loads(lines[0])


def test_more_gpus_than_devices_is_a_json_error_line():
    import torch
    have = torch.cuda.device_count()
    proc = subprocess.run([sys.executable, "bench.py", "--gpus", str(have + 2), "--steps", "1", "--warmup", "0"], capture_output=True, text=True,
                          cwd=ROOT, env=CLEAN, timeout=300)
    d = _one_line(proc)
    assert proc.returncode == 3 and d["value"] is None and d["n_gpus"] == have + 2 and "device(s) visible" in d["error"]


def test_launcher_width_must_equal_gpus():
    env = dict(CLEAN, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    proc = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "1", "--warmup", "0"], capture_output=True, text=True,
                          cwd=ROOT, env=env, timeout=300)
    d = _one_line(proc)
    assert proc.returncode == 2 and "WORLD_SIZE=1" in d["error"]


def test_self_launch_command_is_the_drivers(monkeypatch):
    """self_launch() re-runs the same arguments under `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr
    127.0.0.1 --master-port P bench.py ...` -- the form the driver itself uses for N > 1."""
    import argparse
    import bench
    seen = {}

    class Done:
        returncode = 0

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env
        return Done()

    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7"])

    class FakeCuda:
        @staticmethod
        def device_count():
            return 8

    class FakeTorch:
        cuda = FakeCuda

    args = argparse.Namespace(gpus=4, all_on_device=None, steps=7, warmup=3, scaling="strong", workload="c2")
    assert bench.self_launch(args, FakeTorch) == 0
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    assert cmd[-4:] == ["--gpus", "4", "--steps", "7"] and cmd[-5].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and "MASTER_PORT" not in seen["env"]


def test_stdout_digest_stays_under_8_kb():
    """The driver keeps the last 8 KB of stdout: the ONE line bench.py prints there (slim_line) must carry the contract's fields, `roofline`,
    `cpu_baseline` and every workload's digest inside that -- checked on the full result of a real default run (profiles/r06_bench_full.json)."""
    import bench
    full = json.loads(open(os.path.join(ROOT, "profiles", "r06_bench_full.json")).read())
    line = bench.slim_line(full)
    text = json.dumps(line)
    assert len(text) < 8000, len(text)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in line, k
    assert set(line["roofline"]) >= {"bound", "achieved", "peak", "unit", "frac", "traffic"} and line["cpu_baseline"]["kind"] in ("port", "reference")
    assert set(full["workloads"]) == set(line["workloads"]) and "ragged" in line and line["config"]["workload"].startswith("c2")


def _bits_words(n, seed):
    import numpy as np
    import torch
    bits = np.random.default_rng(seed).random(n) < 0.4
    pad = np.zeros((-n) % 64, dtype=bool)
    return bits, torch.from_numpy(np.packbits(np.concatenate([bits, pad]), bitorder="little").view(np.int64).copy())


def test_dump_outputs_writes_every_row_within_the_budget(tmp_path):
    """--dump-outputs, containedIn: the result bitmap as one float32 0 / 1 per row, every row, no row numbers."""
    import numpy as np
    import bench
    n = 1000
    bits, words = _bits_words(n, 1)
    bench.dump_outputs(str(tmp_path / "d"), words, None, None, n)
    assert sorted(p.name for p in (tmp_path / "d").iterdir()) == ["matched.npy"]
    m = np.load(tmp_path / "d" / "matched.npy")
    assert m.dtype == np.float32 and m.shape == (n,) and (m == bits).all()


def test_dump_outputs_samples_rows_above_the_budget(tmp_path, monkeypatch):
    """--dump-outputs, find(): matched / start / end as float32; above DUMP_MAX_BYTES the same seeded sample of rows from each
    array, its row numbers (sorted, distinct) in row.npy as float64 -- and the same sample on every run."""
    import numpy as np
    import torch
    import bench
    n = 5000
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4 * 3 * n - 1)
    monkeypatch.setattr(bench, "DUMP_SAMPLE_ROWS", 700)
    bits, words = _bits_words(n, 2)
    start = torch.from_numpy(np.where(bits, np.arange(n) % 200, -1).astype(np.int32))
    end = torch.where(start >= 0, start + 5, start)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), words, start, end, n)
    f = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in ("row", "matched", "start", "end")}
    assert f["row"].dtype == np.float64 and all(f[k].dtype == np.float32 for k in ("matched", "start", "end"))
    rows = f["row"].astype(np.int64)
    assert rows.shape == (700,) and (np.diff(rows) > 0).all() and rows[0] >= 0 and rows[-1] < n
    assert (f["matched"] == bits[rows]).all() and (f["start"] == start.numpy()[rows]).all() and (f["end"] == end.numpy()[rows]).all()
    for k in f:
        assert (np.load(tmp_path / "b" / (k + ".npy")) == f[k]).all()


def test_bench_argument_guards_are_json_error_lines(tmp_path):
    """--steps below 1, and --dump-outputs on more than one GPU, stop before any work with ONE error line (exit 2)."""
    for args, msg in ((["--steps", "0"], "--steps must be at least 1"), (["--gpus", "2", "--dump-outputs", str(tmp_path / "d")], "--dump-outputs needs --gpus 1")):
        proc = subprocess.run([sys.executable, "bench.py"] + args, capture_output=True, text=True, cwd=ROOT, env=CLEAN, timeout=300)
        d = _one_line(proc)
        assert proc.returncode == 2 and d["value"] is None and d["error"] == msg
    assert not (tmp_path / "d").exists()
