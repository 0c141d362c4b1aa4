"""bench.py --dump-outputs on the GPU: the timed path's last step, written twice with the same arguments, is the same output file for file; --steps sets
the number of timed steps (a different count is a different last step, hence different rows) and the line carries ms_per_step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench_dump(out, steps):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "bench64", "--steps", str(steps), "--warmup", "1", "--no-cpu-baseline",
                        "--no-latency", "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    return d, {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}


def test_dumped_outputs_repeat_and_follow_the_steps(tmp_path):
    d1, a = bench_dump(tmp_path / "a", 2)
    d2, b = bench_dump(tmp_path / "b", 2)
    d3, c = bench_dump(tmp_path / "c", 3)
    for d, steps in ((d1, 2), (d2, 2), (d3, 3)):
        assert d["valid"] is True and d["steps"] == steps and d["ms_per_step"] > 0
    assert set(a) == {"e", "e_rows", "e_row_sums"} and all(x.dtype == np.float64 for x in a.values())
    assert a["e"].shape == (4096, 932) and (a["e_rows"] == np.arange(4096)).all()         # bench64: 4096 x 932 rows fit the budget whole
    assert (a["e_row_sums"] == a["e"].sum(axis=1)).all()
    assert all((a[k] == b[k]).all() for k in a)
    assert not (a["e"] == c["e"]).all()                   # the last step of three draws with another seed than the last of two
