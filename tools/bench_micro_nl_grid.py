"""Timings of the two cell solvers of -mat_law micro_nl: mcx_homogenize with
every Gauss point yielding, by solver 0 (option micro_nl_solver 0, micro_mem 1: one workgroup per
point) and by solver 1 (grid-wide), and the linear-shortcut test alone on a grid below yield.

    python tools/bench_micro_nl_grid.py --n 10 16 20 --solver 0 1 --points 8 256
    python tools/bench_micro_nl_grid.py --n 32 48 64 --solver 1 --points 8 --ka 1e7
    python tools/bench_micro_nl_grid.py --n 33 --solver 1 --points --linear 16
    python tools/bench_micro_nl_grid.py --n 10 16 --solver 1 --points 8 --start 0 1 --ls 0 5
    python tools/bench_micro_nl_grid.py --n 17 --solver 1 --seed 5 --amp 2e-3 --stages 1 1.5 --start 1 --ls 5
    python tools/bench_micro_nl_grid.py --n 10 16 20 --solver 1 --points 8 256 --ka 1e7 --tangent seq block
    python tools/bench_micro_nl_grid.py --n 10 16 20 32 --solver 1 --points 8 --ka 1e7 --apply split fused
    python tools/bench_micro_nl_grid.py --n 10 16 32 --solver 1 --points 8 --ka 1e7 --tangent seq block --apply fused --warm 0 1

Sphere cells, the tests' load (seed 5; --amp scales it); --ka sets the matrix' hardening modulus (the
cells' plain Newton gives up on resolved cells with the tests' 1e6).  Host clock between two mcx_synchronize;
the second call of each is reported (the first one allocates).  One JSON line per measurement.
--start / --ls list values of the options micro_nl_start / micro_nl_ls, every pair is
measured in the same process; --stages lists load factors with a commit between them, the last one
is the one timed.  A stage whose cells do not converge is reported with the message, not raised.
--tangent lists values of the option micro_nl_tangent (seq, block), measured in the same process.
--apply lists values of the option micro_nl_apply (split, fused), measured in the same process.
--warm lists values of the option micro_nl_warm, measured one after the other in the same
context: per value the timed stage is homogenised three times, at u, at u again and at u x (1 + 1e-3);
the second and the third call are reported (ms, Newton and CG maxima, CG sums), one line per value.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

MAT1, MAT2 = (1.0e7, 0.25, 1.0e4, 1.0e6), (1.0e8, 0.3, 1.0e9, 1.0e7)
GRIDS = {8: (2, 2, 2), 64: (3, 3, 3), 256: (5, 5, 3), 512: (5, 5, 5), 4096: (9, 9, 9)}  # nodes for 8 x elements points


def strain_tensor(e):
    return np.array([[e[0], e[3] / 2, e[4] / 2], [e[3] / 2, e[1], e[5] / 2], [e[4] / 2, e[5] / 2, e[2]]])


def field(grid, seed=5, amp=4e-3, wobble=0.15):
    """u = E0 x plus a nodal wobble on unit elements (the load (5, 4e-3) of the tests)."""
    rng = np.random.default_rng(seed)
    e0 = amp * rng.uniform(-1, 1, 6)
    k, j, i = np.meshgrid(*(np.arange(g, dtype=float) for g in grid[::-1]), indexing="ij")
    X = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1)
    return (X @ strain_tensor(e0).T + wobble * amp * rng.uniform(-1, 1, X.shape)).ravel()


def argv_of(n, grid, ka=MAT1[3], equal=False):
    mat1 = MAT1[:3] + (ka,)
    return ["-da_grid_x", grid[0], "-da_grid_y", grid[1], "-da_grid_z", grid[2], "-lx", grid[0] - 1, "-ly", grid[1] - 1,
            "-lz", grid[2] - 1, "-mat_law", "micro_nl", "-micro_n", n, "-micro_type", 0,
            "-micro_mat_1", "%r,%r,%r,%r" % mat1, "-micro_mat_2", "%r,%r,%r,%r" % (mat1 if equal else MAT2)]


def timed(m, fn):
    m.synchronize()
    t0 = time.perf_counter()
    fn()
    m.synchronize()
    return time.perf_counter() - t0


def warm_rows(m, a, rec, u):
    """option micro_nl_warm: per value, in this context, the calls at u, u and u x (1 + 1e-3); the last two are reported"""
    for warm in a.warm:
        m.set_option("micro_nl_warm", warm)  # 0 releases the records; 1 starts with none valid
        row = dict(rec, warm=warm, converged=True)
        for name, fac in (("first", 1.0), ("second", 1.0), ("third", 1.0 + 1e-3)):
            m.set_u(fac * u)
            m.set_strains()
            dt = timed(m, m.homogenize)
            info = m.micro_nl_info()
            row.update({name + "_ms": dt * 1e3, name + "_newton_max": int(info["newton_its"].max()),
                        name + "_cg_max": int(info["cg_its"].max()), name + "_cg_sum": int(info["cg_its"].sum()),
                        name + "_from_record": int((m.micro_nl_warm() == 2).sum())})
        row.update(solved=int(info["path"].sum()), device_gb=m.get_info()["device_bytes"] / 1e9)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10])
    ap.add_argument("--solver", type=int, nargs="+", default=[0, 1], help="option micro_nl_solver")
    ap.add_argument("--points", type=int, nargs="*", default=[8], help="Gauss points, all yielding: " + str(sorted(GRIDS)))
    ap.add_argument("--amp", type=float, default=4e-3, help="amplitude of the load")
    ap.add_argument("--ka", type=float, default=MAT1[3], help="hardening modulus of the matrix phase")
    ap.add_argument("--equal", action="store_true", help="both phases are the matrix (the cell is the J2 law)")
    ap.add_argument("--seed", type=int, default=5, help="seed of the load")
    ap.add_argument("--stages", type=float, nargs="+", default=[1.0], help="load factors, a commit between them; the last is timed")
    ap.add_argument("--start", type=int, nargs="+", default=[0], help="option micro_nl_start")
    ap.add_argument("--ls", type=int, nargs="+", default=[0], help="option micro_nl_ls")
    ap.add_argument("--tangent", nargs="+", default=["seq"], choices=["seq", "block"], help="option micro_nl_tangent")
    ap.add_argument("--apply", nargs="+", default=["split"], choices=["split", "fused"], help="option micro_nl_apply")
    ap.add_argument("--warm", type=int, nargs="+", default=None, choices=[0, 1], help="option micro_nl_warm: second and third call")
    ap.add_argument("--poll", type=int, default=0, help="option micro_grid_poll (0: leave it alone)")
    ap.add_argument("--linear", type=int, default=0, help="nodes per edge of a macro grid below yield: the linear test alone")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import macroc_amd as M

    for n in a.n:
        for solver in a.solver:
            for pts, start, ls, tangent, apply in [(p, s, k, t, f) for p in a.points for s in a.start for k in a.ls
                                                   for t in a.tangent for f in a.apply]:
                grid = GRIDS[pts]
                u1 = field(grid, seed=a.seed, amp=a.amp)
                rec = dict(tag=a.tag, what="micro_nl", n=n, solver=solver, points=pts, amp=a.amp, seed=a.seed, ka=a.ka,
                           stages=a.stages, equal=a.equal, start=start, ls=ls, tangent=tangent, apply=apply)
                with M.Macroc(argv_of(n, grid, a.ka, a.equal)) as m:
                    m.set_option("micro_mem", 1)
                    m.set_option("micro_nl_solver", solver)
                    if a.poll:
                        m.set_option("micro_grid_poll", a.poll)
                    if start:  # (left alone at 0, so that the tool also runs against a tree without the options)
                        m.set_option("micro_nl_start", start)
                    if ls:
                        m.set_option("micro_nl_ls", ls)
                    if tangent == "block":
                        m.set_option("micro_nl_tangent", 1)
                    if apply == "fused":
                        m.set_option("micro_nl_apply", 1)
                    m.set_option("micro_nl_slots", pts)
                    try:
                        for fac in a.stages[:-1]:
                            m.set_u(fac * u1)
                            m.set_strains()
                            m.homogenize()
                            m.update_vars()
                        if a.warm is not None:
                            warm_rows(m, a, rec, a.stages[-1] * u1)
                            continue
                        m.set_u(a.stages[-1] * u1)
                        m.set_strains()
                        first = timed(m, m.homogenize)
                        dt = timed(m, m.homogenize)
                    except M.MacrocError as e:
                        print(json.dumps(dict(rec, converged=False, message=str(e))), flush=True)
                        continue
                    info = m.micro_nl_info()
                    steps = m.micro_nl_steps() if hasattr(m, "micro_nl_steps") else None
                    dev = m.get_info()["device_bytes"]
                    fused = m.micro_nl_apply_launches() if hasattr(m, "micro_nl_apply_launches") else 0
                solved = int(info["path"].sum())
                cg = info["cg_its"][info["path"] > 0]
                print(json.dumps(dict(rec, converged=True, solved=solved,
                                      first_ms=first * 1e3, ms=dt * 1e3, us_per_point=dt * 1e6 / max(solved, 1),
                                      newton_max=int(info["newton_its"].max()), newton=info["newton_its"].tolist()[:8],
                                      cg_mean=float(cg.mean()) if solved else 0.0,
                                      cg_max=int(info["cg_its"].max()), cg_sum=int(info["cg_its"].sum()),
                                      us_per_cg_it=dt * 1e6 / max(int(info["cg_its"].max()), 1),
                                      rejects=int(steps["ls_rejects"].sum()) if steps else 0,
                                      min_step=float(steps["min_step"][info["path"] > 0].min()) if steps and solved else 1.0,
                                      apply_launches=fused, device_gb=dev / 1e9)), flush=True)
            if a.linear:
                grid = (a.linear,) * 3
                with M.Macroc(argv_of(n, grid, a.ka, a.equal)) as m:
                    m.set_option("micro_mem", 1)
                    m.set_option("micro_nl_solver", solver)
                    m.set_u(field(grid, amp=1e-6))
                    m.set_strains()
                    first = timed(m, m.homogenize)  # with C_hom and the concentration tensors
                    dt = timed(m, m.homogenize)
                    info = m.micro_nl_info()
                gps = 8 * (a.linear - 1) ** 3
                print(json.dumps(dict(tag=a.tag, what="linear_test", n=n, solver=solver, gauss_points=gps,
                                      solved=int(info["path"].sum()), first_ms=first * 1e3, ms=dt * 1e3,
                                      ns_per_gauss_point=dt * 1e9 / gps)), flush=True)


if __name__ == "__main__":
    main()
