"""bench.py on one GPU: a plain run prints the headline line and nothing that needs runs of its own, `--dump-outputs` writes what the last timed
call returned -- exactly, 32-bit halves in float64 -- and that is the CPU oracle's proof of the same statement; `--full` adds the resident-statement
figure and the CPU baseline, whose proof is compared with the GPU's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_N = 14


def _bench(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--log-n", str(LOG_N)] + list(extra),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def _words(path):
    """a dumped array back to the u64 words it holds"""
    x = np.load(path)
    assert x.dtype == np.float64 and np.all(x == np.floor(x)) and x.min() >= 0 and x.max() < 2.0 ** 32
    return np.ascontiguousarray(x.astype(np.uint32)).view(np.uint64)


@pytest.mark.gpu
def test_plain_run_dumps_the_oracle_proof(engine, orc, tmp_path):
    out = _bench("--dump-outputs", str(tmp_path / "dump"))
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(out) and out["steps"] == 2
    assert len(out["ms_per_step_all"]) == 2 and abs(out["ms_per_step"] - sum(out["ms_per_step_all"]) / 2) < 1e-2
    assert abs(out["value"] - (1 << LOG_N) / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
    assert not {"value_resident", "cpu_baseline", "pairing_product_2p16", "msm_g1_2p20", "msm_g2_2p20"} & set(out)
    n = 1 << LOG_N
    a, b, r = orc.gen_g1(1000, n), orc.gen_g2(2000, n), orc.gen_scalars(0, n)
    rc, eproof, ech = orc.sipp_prove(a, b, r, orc.product_of_pairings_with_coeffs(a, b, r))
    assert rc == 0
    assert np.array_equal(_words(tmp_path / "dump" / "proof.npy"), eproof) and np.array_equal(_words(tmp_path / "dump" / "challenges.npy"), ech)


@pytest.mark.gpu
def test_full_run_adds_the_resident_figure_and_the_cpu_baseline(engine):
    out = _bench("--full", "--cpu-log-n", str(LOG_N))
    assert out["value_resident"] > 0 and out["ms_per_step_resident"] > 0
    assert out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["proof_equals_gpu"] is True
