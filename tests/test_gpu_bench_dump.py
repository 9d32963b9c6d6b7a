"""GPU: `bench.py --dump-outputs DIR` writes the state its timed steps computed — the same bits on every run with the same
arguments, the bits of a plain Tau3D run of warmup + steps steps from the same start, and at --gpus 2 the bits of --gpus 1."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def bench_dump(outdir, grid, steps, warmup, *extra, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--grid", str(grid), "--steps", str(steps),
                        "--warmup", str(warmup), "--no-configs", "--no-variants", "--no-cpu-baseline", "--dump-outputs", str(outdir),
                        *extra], capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return {p[:-4]: np.load(os.path.join(outdir, p)) for p in sorted(os.listdir(outdir))}


def same_bits(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert a[k].tobytes() == b[k].tobytes(), f"{k} differs"


@pytest.mark.parametrize("grid", [64, 160])      # 64^3: the whole grid; 160^3 is over the 64 MB budget: the seeded sample
def test_dump_is_the_timed_state_and_repeats(eng, tmp_path, grid):
    import bench
    steps, warmup = 3, 2
    a = bench_dump(tmp_path / "a", grid, steps, warmup)
    same_bits(a, bench_dump(tmp_path / "b", grid, steps, warmup))
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BYTES
    e = eng.Tau3D(grid)
    e.init(1)
    e.set_clock(0.02, 1e-4)
    e.step_async(warmup + steps)
    e.sync()
    clk = e.clock()
    fields = e.download()
    e.close()
    cells = bench.dump_cells(grid)
    assert (cells is None) == (grid == 64)
    for name, f in zip(bench.DUMP_FIELDS, fields):
        want = f if cells is None else f.reshape(-1)[cells]
        assert a[name].dtype == np.float32 and a[name].tobytes() == want.tobytes(), name
    assert a["clock_step"] == clk.step and a["clock_t"] == np.float64(clk.t) and a["clock_maxs"] == np.float64(clk.maxs)


def test_dump_of_two_ranks_equals_one(eng, tmp_path):
    """--gpus 2 on the one shared device (host-staged ring over gloo): each rank contributes its planes' cells"""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", TAU3D_RING_TIMEOUT="120")
    one = bench_dump(tmp_path / "one", 160, 3, 2)
    two = bench_dump(tmp_path / "two", 160, 3, 2, "--gpus", "2", "--ring-transport", "host", env=env)
    same_bits(one, two)
