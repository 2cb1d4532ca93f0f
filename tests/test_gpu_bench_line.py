"""-m gpu: what bench.py's line carries with and without --full.  A plain run is the headline alone (set-up, pre-warm, the timed
regions, --dump-outputs); --full adds the per-kernel, roofline, decode and single-buffer figures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "pipeline", "bit_exact", "kernels", "kernels_overlapped", "decode", "cpu_baseline", "workloads",
             "host_boundary")


def _line(*flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "cfg2", "--steps", "6", "--warmup", "2",
                        "--region-repeats", "3", *flags], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_alone(tmp_path):
    d = _line("--dump-outputs", str(tmp_path / "out"))
    for k in HEADLINE:
        assert k in d, k
    assert d["value"] > 0 and d["higher_is_better"] is True and d["unit"] == "Mpixels/s"
    assert d["ms_per_step"] == d["config"]["region_repeats"]["median"] and d["config"]["region_repeats"]["n"] == 3
    assert d["full"] is False
    assert not [k for k in FULL_ONLY if k in d], d.keys()
    assert "single_input_buffer_ms_per_step" not in d["config"]
    el = d["dump_outputs"]["elements"]
    assert el["block_length"] == d["config"]["code_blocks_per_gpu"]
    for name, n in el.items():
        assert np.load(tmp_path / "out" / (name + ".npy")).size == n


def test_full_run_adds_the_other_figures():
    d = _line("--full", "--no-cpu-baseline", "--no-host-boundary", "--no-live-pmc")
    assert d["full"] is True and d["value"] > 0
    assert d["config"]["single_input_buffer_ms_per_step"] > 0 and d["config"]["coded_bytes_per_gpu"] > 0
    assert d["kernels"]["ht_cleanup_encode"]["avg_ms"] > 0 and d["roofline"]["avg_launch_ms"] > 0
    assert d["decode"]["lossless_round_trip"] is True
    assert d["cpu_baseline"] is None
