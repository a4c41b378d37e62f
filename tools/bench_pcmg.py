"""The Newton system of time step 1 (elastic law, the default load unless --bc-type 0) solved twice on one
context: Jacobi-CG, then PCG around the multigrid V-cycle (-pc_type mg).  Prints one JSON line:
both iteration counts, the multigrid set-up, ms per iteration and per solve of both, and
|du_mg - du_jacobi| / |du_jacobi|.  The first multigrid solve carries the set-up (solve_ms includes
it); a second one on the built hierarchy gives the time per iteration.  --precision single builds the
hierarchy's coarse levels in float (-pc_mg_precision single); --precision both runs the double and the
single hierarchy one after the other on the same context ("mg" and "mg_single")."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import macroc_amd as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--grid", default="256", help="nodes per edge, or NXxNYxNZ")
ap.add_argument("--rtol", type=float, default=1e-8)
ap.add_argument("--bc-type", type=int, default=1, help="1: the load circle (the headline problem), 0: bending")
ap.add_argument("--mat-type", default="aij")
ap.add_argument("--levels", type=int, default=0, help="pc_mg_levels (0: automatic)")
ap.add_argument("--smooth", type=int, default=2, help="pc_mg_smooth (Chebyshev degree)")
ap.add_argument("--no-jacobi", action="store_true", help="skip the Jacobi solves (a profile of the multigrid alone)")
ap.add_argument("--precision", default="double", choices=["double", "single", "both"],
                help="pc_mg_precision; both: the two hierarchies one after the other on this context")
a = ap.parse_args()
g = [int(v) for v in a.grid.split("x")]
g = g * 3 if len(g) == 1 else g
m = M.Macroc(["-da_grid_x", g[0], "-da_grid_y", g[1], "-da_grid_z", g[2], "-bc_type", a.bc_type,
              "-ksp_rtol", repr(a.rtol), "-dm_mat_type", a.mat_type])
m.set_timing(True)
m.apply_bc_on_u(m.get_displacement(0))
m.apply_bc_on_u(m.get_displacement(1))
m.set_strains()
m.homogenize()
m.assembly_res()
m.assembly_jac()
its_j, reason_j, ms_j, du_j = 0, 0, None, None
if not a.no_jacobi:
    m.solve_Ax()  # warm-up: the first solve allocates the p buffers
    its_j, _, reason_j = m.solve_Ax()
    ms_j = m.timing()["solve_ms"]
    du_j = m.du()
bytes_j = m.get_info()["device_bytes"]

m.set_option("pc_mg_levels", a.levels)
m.set_option("pc_mg_smooth", a.smooth)
m.set_option("pc_type", 1)


dus = []


def run_mg(single):
    m.set_option("pc_mg_precision", single)  # a change frees the hierarchy: the next solve builds it
    t0 = time.perf_counter()
    its, rnorm, reason = m.solve_Ax()  # builds the hierarchy
    wall_first = (time.perf_counter() - t0) * 1e3
    ms_first = m.timing()["solve_ms"]
    its2, _, _ = m.solve_Ax()
    ms_mg = m.timing()["solve_ms"]
    du = m.du()
    dus.append(du)
    info = m.pc_mg_info()
    return {"precision": "single" if single else "double", "its": its, "reason": reason, "rnorm": rnorm,
            "levels": info["levels"], "nxyz": info["nxyz"].tolist(), "lmax": info["lmax"].tolist(), "smooth": a.smooth,
            "setup_ms": ms_first - ms_mg, "first_solve_ms": ms_first, "first_solve_wall_ms": wall_first,
            "solve_ms": ms_mg, "ms_per_it": ms_mg / max(its2, 1), "hierarchy_gb": info["bytes"] / 1e9,
            # against Jacobi: null under --no-jacobi
            "speedup_solve": ms_j / ms_mg if ms_j else None, "speedup_first_solve": ms_j / ms_first if ms_j else None,
            "du_rel_diff": float(np.linalg.norm(du - du_j) / np.linalg.norm(du_j)) if du_j is not None else None}


line = {
    "workload": f"{g[0]}x{g[1]}x{g[2]} nodes, time step 1, elastic, bc_type {a.bc_type}, rtol {a.rtol:g}, {a.mat_type}",
    "jacobi": {"its": its_j, "reason": reason_j, "solve_ms": ms_j, "ms_per_it": ms_j / max(its_j, 1)} if ms_j else None,
    "device_gb_jacobi": bytes_j / 1e9,
}
if a.precision != "single":
    line["mg"] = run_mg(0)
if a.precision != "double":
    line["mg_single"] = run_mg(1)
if len(dus) == 2:
    line["du_single_rel_diff"] = float(np.linalg.norm(dus[1] - dus[0]) / np.linalg.norm(dus[0]))
first = line.get("mg", line.get("mg_single"))  # the keys of the one-hierarchy line, as before
line.update(speedup_solve=first["speedup_solve"], speedup_first_solve=first["speedup_first_solve"],
            du_rel_diff=first["du_rel_diff"])
print(json.dumps(line))
m.finish()
