"""Timings of the micro-scale cell solvers: the six unit-strain solves of
-mat_law micro, and mcx_homogenize of -mat_law micro_nl with every Gauss point yielding.

    python tools/bench_micro.py --n 10 12 16 20 --mem 1 --points 8 4096
    python tools/bench_micro.py --n 10 12 16 20 32 64 128 --solver 1 --points

--solver 1 times the grid-wide solver (option micro_solver; -mat_law micro only, so
give --points nothing); its rows add the launches per CG iteration and --poll sets micro_grid_poll.

Host clock between two mcx_synchronize; the second call of each is reported (the first one
allocates).  One JSON line per measurement.  --mem -1 leaves the option alone (a library without
micro_mem); --root selects another checkout's package.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

MAT1, MAT2 = (1.0e7, 0.25, 1.0e4, 1.0e6), (1.0e8, 0.3, 1.0e9, 1.0e7)


def strain_tensor(e):
    return np.array([[e[0], e[3] / 2, e[4] / 2], [e[3] / 2, e[1], e[5] / 2], [e[4] / 2, e[5] / 2, e[2]]])


def field(grid, seed=5, amp=4e-3, wobble=0.15):
    """u = E0 x plus a nodal wobble on unit elements (the load (5, 4e-3) of the tests)."""
    rng = np.random.default_rng(seed)
    e0 = amp * rng.uniform(-1, 1, 6)
    k, j, i = np.meshgrid(*(np.arange(g, dtype=float) for g in grid[::-1]), indexing="ij")
    X = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1)
    return (X @ strain_tensor(e0).T + wobble * amp * rng.uniform(-1, 1, X.shape)).ravel()


def argv_of(law, n, grid):
    return ["-da_grid_x", grid[0], "-da_grid_y", grid[1], "-da_grid_z", grid[2], "-lx", grid[0] - 1, "-ly", grid[1] - 1,
            "-lz", grid[2] - 1, "-mat_law", law, "-micro_n", n, "-micro_type", 0,
            "-micro_mat_1", "%r,%r,%r,%r" % MAT1, "-micro_mat_2", "%r,%r,%r,%r" % MAT2]


def timed(m, fn):
    m.synchronize()
    t0 = time.perf_counter()
    fn()
    m.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10])
    ap.add_argument("--mem", type=int, default=1, help="option micro_mem (-1: leave it alone)")
    ap.add_argument("--solver", type=int, default=0, help="option micro_solver: 0 one workgroup per load case, 1 grid-wide")
    ap.add_argument("--poll", type=int, default=0, help="option micro_grid_poll (0: leave it alone)")
    ap.add_argument("--points", type=int, nargs="*", default=[8, 4096], help="Gauss points of the micro_nl runs")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import macroc_amd as M

    for n in a.n:
        with M.Macroc(argv_of("micro", n, (2, 2, 2))) as m:
            if a.mem >= 0:
                m.set_option("micro_mem", a.mem)
            if a.solver:
                m.set_option("micro_solver", a.solver)
                if a.poll:
                    m.set_option("micro_grid_poll", a.poll)
            m.micro_ctan()
            m.set_option("micro_rtol", 1e-12)  # the default again: marks the cell dirty
            dt = timed(m, m.micro_ctan)
            its = m.micro_ctan()[1]
            dev = m.get_info()["device_bytes"]
        row = dict(tag=a.tag, what="rve", n=n, mem=a.mem, solver=a.solver, ms=dt * 1e3, cg_its=max(its),
                   us_per_cg_it=dt * 1e6 / max(max(its), 1))
        if a.solver:  # five launches per iteration
            row.update(launches_per_cg_it=5, device_gb=dev / 1e9)
        print(json.dumps(row), flush=True)
        for pts in ([] if a.solver else a.points):
            e = round((pts / 8) ** (1.0 / 3.0))
            grid = (e + 1,) * 3
            with M.Macroc(argv_of("micro_nl", n, grid)) as m:
                if a.mem >= 0:
                    m.set_option("micro_mem", a.mem)
                m.set_option("micro_nl_slots", 8 * e ** 3)
                m.set_u(field(grid))
                m.set_strains()
                first = timed(m, m.homogenize)
                dt = timed(m, m.homogenize)
                info = m.micro_nl_info()
                dev = m.get_info()["device_bytes"]
            solved = int(info["path"].sum())
            print(json.dumps(dict(tag=a.tag, what="micro_nl", n=n, mem=a.mem, points=8 * e ** 3, solved=solved,
                                  first_ms=first * 1e3, ms=dt * 1e3, us_per_point=dt * 1e6 / max(solved, 1),
                                  newton=int(info["newton_its"].max()), cg=int(info["cg_its"].max()),
                                  device_gb=dev / 1e9)), flush=True)


if __name__ == "__main__":
    main()
