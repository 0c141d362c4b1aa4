"""bench.py --dump-outputs without a GPU: dump_outputs (the writer the timed path calls) on host arrays -- float64 files, within the 64 MB budget, a seeded
sample of rows that is the same on every run, every row's sum -- and the argument checks of --steps."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRITE = """
import json, sys
import numpy as np
sys.path.insert(0, %r)
import bench
B, m, first, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
e = np.random.default_rng(B + m).integers(-3000, 3000, size=(B, m), dtype=np.int64)
bench.dump_outputs(out, e, first)
np.save(out + ".src.npy", e)
print(json.dumps({"budget": bench.DUMP_BYTES}))
"""


def dump(tmp_path, tag, B, m, first):
    out = str(tmp_path / tag)
    r = subprocess.run([sys.executable, "-c", WRITE % ROOT, str(B), str(m), str(first), out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    budget = json.loads(r.stdout.strip().splitlines()[-1])["budget"]
    files = {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}
    return files, np.load(out + ".src.npy"), sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)), budget


def test_a_large_output_is_a_seeded_sample_within_the_budget(tmp_path):
    B, m, first = 1024, 10000, 4096                      # 82 MB of int64 rows: more than the budget
    files, e, size, budget = dump(tmp_path, "a", B, m, first)
    assert set(files) == {"e", "e_rows", "e_row_sums"}
    assert all(a.dtype == np.float64 for a in files.values())
    assert size <= budget
    rows = files["e_rows"].astype(np.int64) - first
    assert 0 < len(rows) < B and (np.diff(rows) > 0).all() and rows[0] >= 0 and rows[-1] < B
    assert files["e"].shape == (len(rows), m) and (files["e"] == e[rows]).all()
    assert files["e_row_sums"].shape == (B,) and (files["e_row_sums"] == e.sum(axis=1)).all()
    again, _, _, _ = dump(tmp_path, "b", B, m, first)     # same shapes: the same rows, the same files
    assert all((again[k] == files[k]).all() for k in files)


def test_a_small_output_is_written_whole(tmp_path):
    files, e, size, budget = dump(tmp_path, "c", 6, 105, 0)
    assert (files["e_rows"] == np.arange(6)).all() and (files["e"] == e).all() and size <= budget


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 2 and "--steps" in r.stderr and r.stdout.strip() == ""
