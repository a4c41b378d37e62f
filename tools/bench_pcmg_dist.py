"""The Newton system of time step 1 (elastic law, the default load unless --bc-type 0) on a decomposed
grid, solved on every rank's context twice: Jacobi-CG, then PCG around the distributed multigrid
V-cycle (-pc_mg_dist 1 -pc_type mg).  The ranks are contexts of one in-process group on one GPU, one
host thread each (BASELINE config 4's workload is --grid 512 --procs 2x2x2).  Prints one JSON line: both
iteration counts, the multigrid set-up, ms per iteration and per solve of both, the bytes per rank,
|du_mg - du_jacobi| / |du_jacobi| over all ranks, and the halo exchanges and all-reduces of one PCG
iteration (counted from the cycle's definition).

The in-process transport serialises the ranks on one device: its time per iteration says nothing
about as many GPUs.  What carries over is the iteration count, the memory and the counts of
collectives.  --precision single keeps the coarse levels in float (-pc_mg_precision single); both
runs the double and the single hierarchy one after the other on the same contexts ("mg", "mg_single")."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import macroc_amd as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--grid", default="512", help="global nodes per edge, or NXxNYxNZ")
ap.add_argument("--procs", default="2x2x2", help="rank grid")
ap.add_argument("--rtol", type=float, default=1e-8)
ap.add_argument("--bc-type", type=int, default=1, help="1: the load circle (the headline problem), 0: bending")
ap.add_argument("--levels", type=int, default=0, help="pc_mg_levels (0: automatic)")
ap.add_argument("--smooth", type=int, default=2, help="pc_mg_smooth (Chebyshev degree)")
ap.add_argument("--no-jacobi", action="store_true", help="skip the Jacobi solves (thousands of iterations at 512^3)")
ap.add_argument("--comm-timeout", type=float, default=300.0)
ap.add_argument("--precision", default="double", choices=["double", "single", "both"],
                help="pc_mg_precision; both: the two hierarchies one after the other on these contexts")
a = ap.parse_args()
g = [int(v) for v in a.grid.split("x")]
g = g * 3 if len(g) == 1 else g
p = [int(v) for v in a.procs.split("x")]
nr = p[0] * p[1] * p[2]
argv = ["-da_grid_x", g[0], "-da_grid_y", g[1], "-da_grid_z", g[2], "-da_processors_x", p[0], "-da_processors_y", p[1],
        "-da_processors_z", p[2], "-bc_type", a.bc_type, "-ksp_rtol", repr(a.rtol)]
PRECISIONS = {"double": [0], "single": [1], "both": [0, 1]}[a.precision]
group = M.LocalGroup(nr)
out, errors = [None] * nr, []


def rank_main(r):
    try:
        m = M.Macroc(argv, rank=r, nranks=nr, group=group)
        try:
            o = {}
            m.set_option("comm_timeout", a.comm_timeout)
            m.set_timing(True)
            m.apply_bc_on_u(m.get_displacement(0))
            m.apply_bc_on_u(m.get_displacement(1))
            m.set_strains()
            m.homogenize()
            m.assembly_res()
            m.assembly_jac()
            if not a.no_jacobi:
                m.solve_Ax()  # warm-up: the first solve allocates the p buffers
                o["its_j"], _, o["reason_j"] = m.solve_Ax()
                o["ms_j"] = m.timing()["solve_ms"]
                o["du_j"] = m.du()
            o["bytes_j"] = m.get_info()["device_bytes"]
            m.set_option("pc_mg_dist", 1)
            m.set_option("pc_mg_levels", a.levels)
            m.set_option("pc_mg_smooth", a.smooth)
            m.set_option("pc_type", 1)
            o["mg"] = {}
            for single in PRECISIONS:
                q = o["mg"][single] = {}
                m.set_option("pc_mg_precision", single)  # a change frees the hierarchy: the next solve builds it
                t0 = time.perf_counter()
                q["its"], q["rnorm"], q["reason"] = m.solve_Ax()  # builds the hierarchy
                q["wall_first"] = (time.perf_counter() - t0) * 1e3
                q["ms_first"] = m.timing()["solve_ms"]
                q["its2"] = m.solve_Ax()[0]
                q["ms_mg"] = m.timing()["solve_ms"]
                q["du"] = m.du()
                q["info"] = m.pc_mg_info()
            o["box1"] = [int(v) for v in m.pc_mg_box(1)[1]]
            out[r] = o
        finally:
            m.finish()
    except Exception as e:  # reported below
        errors.append((r, repr(e)))


ts = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(nr)]
for t in ts:
    t.start()
for t in ts:
    t.join()
if errors:
    sys.exit(f"bench_pcmg_dist: {errors}")
group.destroy()
k = a.smooth


def mg_line(single):
    qs = [o["mg"][single] for o in out]
    q0, info = qs[0], qs[0]["info"]
    L = info["levels"]
    return {"precision": "single" if single else "double", "its": q0["its"], "reason": q0["reason"], "rnorm": q0["rnorm"],
            "levels": L, "nxyz": info["nxyz"].tolist(),
            "lmax": info["lmax"].tolist(), "smooth": k, "setup_ms": max(q["ms_first"] - q["ms_mg"] for q in qs),
            "first_solve_ms": max(q["ms_first"] for q in qs), "first_solve_wall_ms": max(q["wall_first"] for q in qs),
            "solve_ms": max(q["ms_mg"] for q in qs), "ms_per_it": max(q["ms_mg"] for q in qs) / max(q0["its2"], 1),
            "same_on_every_rank": all((q["its"], q["rnorm"], q["reason"]) == (q0["its"], q0["rnorm"], q0["reason"]) for q in qs),
            "hierarchy_bytes_per_rank": [q["info"]["bytes"] for q in qs], "level1_box_per_rank": [o["box1"] for o in out],
            # per PCG iteration: every smoothed level fills x's ghosts before each of its 2k operator
            # applications (k - 1 in the pre-smoother, the residual, k in the post-smoother), the masked
            # residual's before P^T and, unless the coarsest level sits below, the correction's before P; the
            # search direction's before the fine SpMV.  All-reduces: r.z, p.Ap and the coarsest right-hand side
            "halo_exchanges_per_it": (L - 1) * (2 * k + 1) + (L - 2) + 1, "allreduces_per_it": 3}


line = {
    "workload": f"{g[0]}x{g[1]}x{g[2]} nodes over {p[0]}x{p[1]}x{p[2]} ranks (in-process transport, one GPU), time step 1, "
                f"elastic, bc_type {a.bc_type}, rtol {a.rtol:g}",
    "device_bytes_per_rank_jacobi": [o["bytes_j"] for o in out],
    "note": "the in-process transport serialises the ranks on one device: ms per iteration is no multi-GPU figure",
}
for single in PRECISIONS:
    line["mg_single" if single else "mg"] = mg_line(single)
if len(PRECISIONS) == 2:
    dd, ds = (np.concatenate([o["mg"][s]["du"] for o in out]) for s in PRECISIONS)
    line["du_single_rel_diff"] = float(np.linalg.norm(ds - dd) / np.linalg.norm(dd))
if not a.no_jacobi:
    first = PRECISIONS[0]  # the keys of the one-hierarchy line, as before
    dj = np.concatenate([o["du_j"] for o in out])
    dm = np.concatenate([o["mg"][first]["du"] for o in out])
    ms_j = max(o["ms_j"] for o in out)
    mgl = line["mg_single" if first else "mg"]
    line["jacobi"] = {"its": out[0]["its_j"], "reason": out[0]["reason_j"], "solve_ms": ms_j, "ms_per_it": ms_j / max(out[0]["its_j"], 1)}
    line["speedup_solve"] = ms_j / mgl["solve_ms"]
    line["speedup_first_solve"] = ms_j / mgl["first_solve_ms"]
    line["du_rel_diff"] = float(np.linalg.norm(dm - dj) / np.linalg.norm(dj))
print(json.dumps(line))
