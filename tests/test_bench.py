"""bench.py's own contract: a plain run prints the headline line only, --dump-outputs writes the last timed step's outputs
(float64 .npy, at most 64 MB in all) from seeded inputs, and --full adds the other legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "roofline_em_iteration", "roofline_em_sweep", "roofline_class_build", "host_pinned", "value_host_pinned",
             "sampling", "cpu_baseline", "parity_vs_cpu", "speedup_vs_cpu")


def _bench(*args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_dump_outputs_keeps_to_the_size_limit(tmp_path):
    import bench
    small = {"x": np.arange(10.0), "y": np.arange(7, dtype=np.int64)}
    bench.dump_outputs(str(tmp_path / "s"), small)
    for k, v in small.items():
        got = np.load(tmp_path / "s" / f"{k}.npy")
        assert got.dtype == np.float64 and np.array_equal(got, v)
    big = {"a": np.arange(6_000_000.0), "b": np.arange(6_000_000.0) * 2, "c": np.ones(10)}
    for d in ("b1", "b2"):
        bench.dump_outputs(str(tmp_path / d), big)
    total = sum(os.path.getsize(tmp_path / "b1" / f"{k}.npy") for k in big)
    assert total <= bench.DUMP_LIMIT_BYTES
    a1, a2, b1 = (np.load(tmp_path / d / f"{k}.npy") for d, k in (("b1", "a"), ("b2", "a"), ("b1", "b")))
    assert np.array_equal(a1, a2) and np.array_equal(b1, 2 * a1)          # a fixed sample: the same positions every time
    assert np.all(np.diff(a1) > 0) and np.load(tmp_path / "b1" / "c.npy").size == 10


@pytest.mark.gpu
def test_plain_run_and_its_outputs(gpu, tmp_path):
    outs = []
    for i in range(2):
        d = _bench("--gpus", "1", "--workload", "small", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / f"o{i}"))
        assert d["steps"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "reads/s"
        assert d["higher_is_better"] is True and d["dtype"] == "f64"
        assert abs(d["value"] - d["config"]["reads_total"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
        assert not [k for k in FULL_ONLY if k in d], d.keys()
        o = {k: np.load(tmp_path / f"o{i}" / f"{k}.npy") for k in ("num_reads", "tpm", "effective_length", "class_counts", "class_label_lengths")}
        assert all(v.dtype == np.float64 for v in o.values())
        M, C = d["config"]["transcripts"], d["config"]["classes"]
        assert o["num_reads"].size == o["tpm"].size == o["effective_length"].size == M
        assert o["class_counts"].size == o["class_label_lengths"].size == C
        assert o["class_label_lengths"].sum() == d["config"]["nnz"]
        assert o["class_counts"].sum() == d["config"]["reads_total"]
        assert abs(o["num_reads"].sum() - d["config"]["reads_total"]) < 1e-4 * d["config"]["reads_total"]
        assert abs(o["tpm"].sum() - 1e6) < 1e-2
        outs.append(o)
    # seeded inputs: the same classes, and the same estimates, run after run
    for k in ("class_counts", "class_label_lengths", "effective_length"):
        assert np.array_equal(outs[0][k], outs[1][k]), k
    nz = outs[0]["num_reads"] > 0
    assert np.array_equal(outs[1]["num_reads"] > 0, nz)
    assert np.max(np.abs(outs[1]["num_reads"][nz] - outs[0]["num_reads"][nz]) / outs[0]["num_reads"][nz]) < 1e-6


@pytest.mark.gpu
def test_full_run_adds_the_other_legs(gpu):
    d = _bench("--gpus", "1", "--workload", "small", "--steps", "2", "--warmup", "1", "--full", "--cpu-seconds", "1",
               "--gibbs-draws", "64", "--bootstrap-draws", "2")
    assert d["steps"] == 2 and d["value"] > 0
    for k in ("roofline", "roofline_em_iteration", "roofline_em_sweep", "roofline_class_build", "value_host_pinned", "sampling",
              "cpu_baseline", "parity_vs_cpu"):
        assert k in d, k
    assert d["host_pinned"].get("same_result_as_hbm_resident_step") is True
    assert "error" not in d["parity_vs_cpu"] and d["parity_vs_cpu"]["classes_identical"]
