"""bench.py --dump-outputs on the GPU: two runs of the same workload with other step counts write the same outputs (the inputs
are seeded, the sample is fixed), and the line reports the steps that were asked for."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(tmp_path, name, steps, warmup):
    out = tmp_path / name
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "small", "--steps", str(steps),
           "--warmup", str(warmup), "--no-live-pmc", "--no-extras", "--no-cpu-baseline", "--no-bandwidth", "--secondary-depth",
           "0", "--side-file", str(tmp_path / f"{name}_side.json"), "--dump-outputs", str(out)]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_same_from_run_to_run(tmp_path):
    d1, a = _bench(tmp_path, "a", 3, 1)
    d2, b = _bench(tmp_path, "b", 1, 0)
    assert (d1["steps"], d1["warmup"], d2["steps"], d2["warmup"]) == (3, 1, 1, 0)
    assert d1["ms_per_step"] > 0 and d2["ms_per_step"] > 0
    assert sorted(a) == sorted(b) == ["counts", "hit_index", "hit_offsets", "hit_position", "hit_text_id", "query_index", "status",
                                      "totals"]
    assert sum(x.nbytes for x in a.values()) <= 64 << 20 and all(x.dtype in (np.float32, np.float64) for x in a.values())
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    nq, total = a["totals"].tolist()
    assert nq == d1["config"]["queries_per_gpu"] and total == d1["config"]["hits_per_gpu"]
    assert np.all(a["hit_offsets"] + a["counts"] <= total) and np.all(a["hit_index"] < total)
    assert np.all(np.diff(a["hit_offsets"]) >= a["counts"][:-1]) and a["counts"].sum() > 0


@pytest.mark.gpu
def test_plain_bench_run_measures_the_headline_alone(tmp_path):
    """Without --full the run sets up, warms up, times the steps and prints the line: no PMC passes, no other input form, no
    shard steps, no hit check, no bandwidths, no CPU baseline, no end to end, no secondaries."""
    side = tmp_path / "side.json"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "small", "--steps", "2", "--warmup", "1",
           "--side-file", str(side)]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert (d["n_gpus"], d["steps"], d["warmup"], d["scaling"], d["unit"], d["dtype"]) == (1, 2, 1, "weak", "queries/s", "u32")
    assert d["higher_is_better"] is True and d["ms_per_step"] > 0
    assert abs(d["value"] - d["config"]["queries_per_gpu"] / (d["ms_per_step"] / 1e3)) < 1e-4 * d["value"]
    assert d["cpu_baseline"] is None and d["roofline"]["traffic"] is None and d["roofline"]["frac"] is None
    assert d["kernel_ms"]["search"] > 0 and d["config"]["hits_per_gpu"] > 0
    full = json.load(open(side))
    assert full["ascii_input"] is None and full["packed_input"] is None and full["shard_step"] is None
    assert full["locate_roofline"] is None and set(full["parity"]) == {"queries_with_status"}
    assert not {"measured_bandwidth", "end_to_end", "secondary"} & set(full)
    assert "live PMC" not in res.stderr
