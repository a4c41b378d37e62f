"""bench.py's command line on a CPU host: --full and --dump-outputs exist, and the dump writes
float64 arrays, whole when small and the same seeded sample in every run when large."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_help_names_full_and_dump_outputs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "--full" in out.stdout and "--dump-outputs DIR" in out.stdout


def test_dump_outputs_whole_and_sampled(tmp_path):
    import bench

    small = np.arange(30, dtype=np.float64)
    big = np.sin(np.arange(bench.DUMP_SAMPLE + 1000, dtype=np.float64))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), 0, 1, 1.5, 7, 2.5e-9, 2, small, big)
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("step", "u", "du")}
    b = {n: np.load(tmp_path / "b" / f"{n}.npy") for n in ("step", "u", "du")}
    assert sorted(os.listdir(tmp_path / "a")) == ["du.npy", "step.npy", "u.npy"]
    assert all(v.dtype == np.float64 for v in a.values())
    assert np.array_equal(a["step"], [1.5, 7.0, 2.5e-9, 2.0])
    assert np.array_equal(a["u"], small)
    assert a["du"].shape == (bench.DUMP_SAMPLE,) and np.isin(a["du"], big).all()
    assert all(np.array_equal(a[n], b[n]) for n in a)
    # u and du at the sample size, float64, stay far below the 64 MB a dump may take
    assert 2 * bench.DUMP_SAMPLE * 8 + 4 * 8 < 64e6
    bench.dump_outputs(str(tmp_path / "r"), 3, 8, 0.0, 0, 0.0, 2, small, small)
    assert sorted(os.listdir(tmp_path / "r")) == ["du_rank3.npy", "step_rank3.npy", "u_rank3.npy"]
