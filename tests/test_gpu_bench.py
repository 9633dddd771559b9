"""GPU: the plain `bench.py` run -- K timed steps, ONE JSON line without the `--full` legs, and `--dump-outputs` writing
what the last timed step computed, checked against the CPU oracle on the same arrays (bench.py's config Cm inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import gp_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cm_minibatch(step):
    """bench.make_inputs for config Cm (N = 1e6, M = 2048, D = 8, seed 4), re-derived on the host; rows of minibatch `step`."""
    n, m, d, b = 1_000_000, 2048, 8, 8192
    rng = np.random.default_rng(4)
    X = rng.standard_normal((n, d))
    Y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((n, 1))
    Z = X[:m] + 0.01 * rng.standard_normal((m, d))
    q_mu = 0.1 * rng.standard_normal((m, 1))
    q_sqrt = np.tril(0.05 * rng.standard_normal((1, m, m))) + 0.5 * np.eye(m)
    lo = (step % (n // b)) * b
    return X[lo:lo + b], Y[lo:lo + b], Z, q_mu, q_sqrt, np.sqrt(d) * (0.8 + 0.05 * np.arange(d))


@pytest.mark.gpu
def test_plain_bench_times_k_steps_and_dumps_the_last_step(gpu, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out_dir = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["metric"] == "svgp_elbo_steps_per_s" and rec["unit"] == "steps/s" and rec["higher_is_better"] is True
    assert rec["dtype"] == "f64" and rec["steps"] == 3 and rec["warmup"] == 2 and rec["full"] is False
    assert rec["ms_per_step"] > 0 and abs(rec["value"] * rec["ms_per_step"] - 1e3) <= 1e-6 * 1e3
    for leg in ("roofline", "stream_selfcheck", "cpu_baseline", "train_step", "other_workloads", "gpr_cholesky"):
        assert leg not in rec, leg
    assert rec["dumped_outputs"] == ["elbo", "elbo_terms"]
    elbo, terms = np.load(out_dir / "elbo.npy"), np.load(out_dir / "elbo_terms.npy")
    assert elbo.dtype == np.float64 and elbo.shape == (1,) and terms.dtype == np.float64 and terms.shape == (2,)
    assert float(elbo[0]) == rec["last_elbo"]
    assert abs(terms[0] * (1_000_000 / 8192) - terms[1] - elbo[0]) <= 1e-12 * abs(elbo[0])
    # the last timed step is step warmup + steps - 1 = 4
    Xb, Yb, Z, q_mu, q_sqrt, ls = _cm_minibatch(4)
    ref = orc.svgp_elbo(Xb, Yb, Z, q_mu, q_sqrt, variance=1.0, lengthscales=ls, noise_variance=0.1, whiten=True,
                        num_data=1_000_000)
    assert abs(float(elbo[0]) - ref) <= 1e-8 * abs(ref), (float(elbo[0]), ref)
