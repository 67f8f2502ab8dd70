"""bench.py --dump-outputs DIR: the records the timed path's last step handed to the caller, as DIR/<name>.npy.
CPU: the writer (every array as computed; beyond the size cap the same seeded sample of environments) and --steps.
GPU: the driver's own workload — two runs with the same arguments dump the same arrays, and so do the same steps split
differently between warm-up and timed region, and the same steps as eager single-step launches."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, rel_err

import bench
import tds_amd


def test_dump_outputs_writes_every_array_as_computed(tmp_path):
    rng = np.random.default_rng(1)
    arrays = {"y": rng.normal(size=(64, 155)), "obs": rng.normal(size=(64, 30)).astype(np.float32)}
    bench.dump_outputs(str(tmp_path / "d"), arrays)
    for k, a in arrays.items():
        b = np.load(tmp_path / "d" / (k + ".npy"))
        assert b.dtype == a.dtype and np.array_equal(a, b), k


def test_dump_outputs_samples_the_same_environments_within_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 64000)
    n = 1000
    y = np.repeat(np.arange(n, dtype=np.float64)[:, None], 20, axis=1)   # row e holds e
    obs = np.repeat(np.arange(n, dtype=np.float32)[:, None], 8, axis=1)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"y": y, "obs": obs})
    ya, oa = np.load(tmp_path / "a" / "y.npy"), np.load(tmp_path / "a" / "obs.npy")
    assert 0 < ya.nbytes + oa.nbytes <= bench.DUMP_BYTES
    assert np.array_equal(ya[:, 0].astype(np.float32), oa[:, 0])       # the same environments in every array
    assert (np.diff(ya[:, 0]) > 0).all() and (ya == ya[:, :1]).all()    # whole rows, distinct, in order
    assert np.array_equal(ya, np.load(tmp_path / "b" / "y.npy"))        # the same sample from run to run
    assert np.array_equal(oa, np.load(tmp_path / "b" / "obs.npy"))


def test_help_names_the_option():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "--dump-outputs DIR" in p.stdout


def test_steps_below_one_are_refused():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 2 and "--steps" in p.stderr


@pytest.mark.gpu
def test_dump_outputs_of_the_timed_path(tmp_path, built):
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--no-cpu-baseline", "--no-secondary",
            "--spin-up-steps", "0"]

    def run(tag, *extra):
        d = tmp_path / tag
        p = subprocess.run(base + list(extra) + ["--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        line = json.loads(p.stdout.strip().splitlines()[-1])
        assert sorted(os.listdir(d)) == ["obs.npy", "y.npy"]
        return line, {k: np.load(d / (k + ".npy")) for k in ("y", "obs")}

    la, a = run("a", "--steps", "20", "--warmup", "5")
    lb, b = run("b", "--steps", "20", "--warmup", "5")
    lc, c = run("c", "--steps", "25", "--warmup", "0")          # the same 25 steps, all of them timed
    ld, d = run("d", "--steps", "25", "--warmup", "0", "--no-graph")   # ... as 25 single-step launches
    assert (la["steps"], lb["steps"], lc["steps"], ld["steps"]) == (20, 20, 25, 25)
    assert la["ms_per_step"] > 0 and la["config"]["per_step_records"]
    m = tds_amd.load_model("ant")
    assert a["y"].shape == (4096, m.output_dim) and a["y"].dtype == np.float64
    assert a["obs"].shape[0] == 4096 and a["obs"].dtype == np.float64
    assert np.isfinite(a["y"]).all() and np.isfinite(a["obs"]).all()
    for k in ("y", "obs"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
        assert rel_err(d[k], a[k]) < 1e-12, k
