"""bench.py's plain run, its --full run and --dump-outputs: what the last timed step computed, on inputs that are the same
from run to run, as float32 / float64 .npy files of 64 MB at most."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, capture_output=True, text=True,
                          timeout=timeout)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_whole_or_a_fixed_sample(tmp_path):
    import torch

    import bench

    big = torch.rand(160_000, 84)  # 53.8 MB: beyond the sample budget
    path = torch.randint(-1, 5000, (8, 100), dtype=torch.int32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"posteriors": big.reshape(1000, 160, 84), "total_loglik": torch.randn(1000).double(),
                                               "path": path, "loss": torch.tensor(1.5)})
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["loss", "path", "posteriors", "posteriors_rows", "total_loglik"]
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_BYTES
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    rows = a["posteriors_rows"].astype(np.int64)
    assert np.array_equal(rows, b["posteriors_rows"]) and (np.diff(rows) > 0).all() and rows[-1] < 160_000
    assert np.array_equal(a["posteriors"], big.numpy()[rows])
    assert a["path"].dtype == np.float64 and np.array_equal(a["path"], path.numpy())  # (int32 states: exact in float64)
    assert a["loss"].shape == () and a["loss"] == np.float32(1.5)


def test_bench_rejects_no_timed_steps():
    r = _bench("--steps", "0", timeout=60)
    assert r.returncode == 2 and "--steps" in r.stderr
    assert not any(ln.startswith("{") for ln in r.stdout.splitlines())


@pytest.mark.gpu
def test_plain_bench_dumps_the_last_step(tmp_path):
    """Two plain runs with different step counts: `steps` is what was asked, the line has no --full record, and the outputs
    are the same (same inputs): per-frame posteriors that sum to one, finite log-likelihoods."""
    outs = []
    for steps, d in ((3, "a"), (5, "b")):
        r = _bench("--gpus", "1", "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(tmp_path / d))
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == steps and line["ms_per_step"] > 0 and line["metric"] == "pdfposteriors_frames_per_sec"
        assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert abs(line["value"] * line["ms_per_step"] * 1e-3 - 256 * 1500) < 1.0
        assert not {"sharp", "sharp_consistent", "cpu_baseline"} & set(line)
        outs.append(_load(tmp_path / d))
    a, b = outs
    assert sorted(a) == ["posteriors", "posteriors_rows", "total_loglik"]
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert a["total_loglik"].shape == (256,) and np.isfinite(a["total_loglik"]).all()
    assert a["posteriors"].shape[1] == 84 and np.allclose(a["posteriors"].sum(1), 1.0, atol=1e-4)
    assert np.array_equal(a["posteriors_rows"], b["posteriors_rows"])
    assert np.allclose(a["posteriors"], b["posteriors"], rtol=1e-5, atol=1e-7)
    assert np.allclose(a["total_loglik"], b["total_loglik"], rtol=1e-6)


@pytest.mark.gpu
def test_full_bench_keeps_the_sharp_records():
    r = _bench("--gpus", "1", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline")
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["sharp"]["finite"] and line["sharp_consistent"]["finite"]
    assert "posterior_floor_1e-12" in line["sharp_consistent"]
