"""bench.py contract: runs on one GPU and prints the JSON line."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_dump(dump):
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
         "--steps", "3", "--warmup", "2", "--batch", "256",
         "--dump-outputs", str(dump)],
        capture_output=True,
        text=True,
        timeout=600,
        cwd=ROOT,
    )
    return r


@pytest.fixture(scope="module")
def bench_run(tmp_path_factory):
    dump = tmp_path_factory.mktemp("bench") / "dump"
    return _bench_dump(dump), dump


def test_bench_single_gpu_json(bench_run):
    r, dump = bench_run
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["unit"] == "samples/sec"
    assert d["n_gpus"] == 1
    assert d["steps"] == 3
    assert d["value"] > 0
    assert d["dtype"] == "bf16"
    assert d["data"] == "synthetic"
    assert d["higher_is_better"] is True
    assert d["config"]["model"] == "resnet18-cifar"
    assert d["loss"] == d["loss"]  # not NaN
    assert d["ms_per_step"] > 0
    assert d["full"] is False
    # --dump-outputs: the timed step re-run from the seeded initial state,
    # as float32 .npy
    loss = np.load(dump / "loss.npy")
    logits = np.load(dump / "logits.npy")
    params = np.load(dump / "params.npy")
    assert loss.dtype == logits.dtype == params.dtype == np.float32
    # one step from random init on 10 classes: near ln(10)
    assert loss.shape == (1,) and 1.5 < float(loss[0]) < 4.0
    assert logits.shape == (256, 10)
    assert params.ndim == 1 and params.size > 10_000_000  # all of ResNet-18
    assert np.isfinite(logits).all() and np.isfinite(params).all()
    assert loss.nbytes + logits.nbytes + params.nbytes <= 64 << 20


def test_bench_dump_reproducible(bench_run, tmp_path):
    """Two runs with the same arguments dump the same arrays up to rounding.
    The step computes in bf16 (8-bit significand, one ulp = 2^-8 relative)
    and the only run-to-run freedom is the order of fp32 atomic sums, which
    can move a bf16 result by an ulp here and there — so the rms difference
    over an array must stay below one bf16 ulp of the array's rms, and the
    fp32 loss within 1e-3 relative."""
    r1, dump1 = bench_run
    assert r1.returncode == 0, r1.stderr[-2000:]
    dump2 = tmp_path / "dump"
    r2 = _bench_dump(dump2)
    assert r2.returncode == 0, r2.stderr[-2000:]
    for name, bound in (("loss", 1e-3), ("logits", 2.0 ** -8),
                        ("params", 2.0 ** -8)):
        a = np.load(dump1 / (name + ".npy")).astype(np.float64)
        b = np.load(dump2 / (name + ".npy")).astype(np.float64)
        assert a.shape == b.shape
        rel = np.linalg.norm(a - b) / np.linalg.norm(a)
        print(f"{name}: rel l2 diff {rel:.3e} (bound {bound:.3e})")
        assert rel <= bound, (name, rel)


def _bench_loss(extra):
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
         "--steps", "6", "--warmup", "3", "--batch", "512"] + extra,
        capture_output=True, text=True, timeout=600, cwd=ROOT,
    )
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line)["loss"]


def test_bench_graph_matches_eager_semantics():
    """The hipGraph-captured step must run the SAME training math as the
    eager step: identical seeds/data give closely matching final losses
    (loose tolerance: the wgrad fp32 atomics make reduction order, and
    hence bf16 rounding, nondeterministic across any two runs).  This is
    the regression guard for capture bugs that silently freeze weights or
    skip work — a frozen capture pins loss near ln(10)=2.30 while eager
    descends."""
    lg = _bench_loss([])           # graph default at N=1
    le = _bench_loss(["--no-graph"])
    assert abs(lg - le) < 0.35, (lg, le)
