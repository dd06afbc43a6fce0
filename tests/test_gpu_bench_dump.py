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
