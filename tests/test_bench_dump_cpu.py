"""bench.py's `--dump-outputs` writer and argument checks, without a GPU.  bench.py is driven in a child process: importing it sets
HSA variables that must not reach this test process."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WRITE = """
import json, sys
import numpy as np
import bench
rng = np.random.default_rng(1)
k, n = 4, 1000
e, f, x = rng.standard_normal(k), rng.standard_normal((k, 3 * n)), rng.standard_normal((k, 3 * n))
np.savez(sys.argv[1], e=e, f=f, x=x)
print(json.dumps([bench.dump_outputs(d, e, f, x, limit=int(lim)) for d, lim in zip(sys.argv[2::2], sys.argv[3::2])]))
"""


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, n)) for n in os.listdir(d))


def test_dump_outputs_whole_and_sampled(tmp_path):
    """Below the limit the arrays are written whole; above it the per-atom arrays keep a seeded sample of atoms, the same one on every
    call, and everything written (the sampled atom indices included) stays within the limit."""
    src = str(tmp_path / "src.npz")
    whole, s1, s2 = (str(tmp_path / d) for d in ("whole", "s1", "s2"))
    limit = 40000
    out = subprocess.run([sys.executable, "-c", WRITE, src, whole, str(64 << 20), s1, str(limit), s2, str(limit)], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    info = json.loads(out.stdout.strip().splitlines()[-1])
    ref = np.load(src)
    e, f, x = ref["e"], ref["f"].reshape(4, -1, 3), ref["x"].reshape(4, -1, 3)

    assert info[0]["atom_sample"] is None and info[0]["arrays"] == {"energy": [4], "forces": [4, 1000, 3], "string": [4, 1000, 3]}
    assert sorted(os.listdir(whole)) == ["energy.npy", "forces.npy", "string.npy"]
    for name, want in (("energy", e), ("forces", f), ("string", x)):
        got = np.load(os.path.join(whole, name + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, want), name

    m = info[1]["atom_sample"]["atoms"]
    assert 0 < m < 1000 and info[1]["atom_sample"]["of"] == 1000 and info[1]["atom_sample"] == info[2]["atom_sample"]
    idx = np.load(os.path.join(s1, "atom_index.npy"))
    assert idx.dtype == np.float64 and idx.shape == (m,) and np.all(np.diff(idx) > 0)
    i = idx.astype(np.int64)
    assert np.array_equal(np.load(os.path.join(s1, "forces.npy")), f[:, i]) and np.array_equal(np.load(os.path.join(s1, "string.npy")), x[:, i])
    assert np.array_equal(np.load(os.path.join(s1, "energy.npy")), e)
    for name in ("energy", "forces", "string", "atom_index"):
        assert np.array_equal(np.load(os.path.join(s1, name + ".npy")), np.load(os.path.join(s2, name + ".npy"))), name
    # the .npy headers are not counted by the writer: allow them on top of the limit
    assert _dir_bytes(s1) - limit <= 4 * 128 and sum(np.load(os.path.join(s1, n)).nbytes for n in os.listdir(s1)) <= limit


def test_bench_rejects_no_timed_steps():
    """`--steps` is the number of timed steps: zero would leave nothing to time (and ms_per_step undefined)."""
    for args in (["--steps", "0"], ["--warmup", "-1"]):
        out = subprocess.run([sys.executable, "bench.py", *args], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert out.returncode == 2 and "--steps must be >= 1" in out.stderr, (args, out.stderr[-2000:])
