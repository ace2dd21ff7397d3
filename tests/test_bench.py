"""bench.py's result line: a plain run carries the headline alone, --full adds the golden parity (and, with its other
options, the CPU legs and the `secondary` records)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1"]
                       + list(args), cwd=ROOT, stdout=subprocess.PIPE, timeout=300, check=True)
    lines = p.stdout.decode().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_line_is_the_headline_alone():
    d = _bench()
    assert d["metric"] == "LPs solved/sec" and d["unit"] == "LPs/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["solved_optimal"] == 65536 and d["roofline"]["kernel_ms"] > 0
    assert d["parity"] is None and d["cpu_baseline"] is None and d["cpu_port"] is None and "secondary" not in d


@pytest.mark.gpu
def test_full_bench_line_carries_the_golden_parity():
    d = _bench("--full", "--no-cpu-baseline", "--no-secondary")
    assert d["parity"]["ok"] and d["parity"]["golden_lps"] > 0
    assert d["cpu_baseline"] is None and "secondary" not in d
