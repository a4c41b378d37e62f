"""Generator of the resolved-cell fixtures tests/golden/cell_*.npz ("Resolved cells against the
sparse reference").

tests/micro_cell_sparse_ref.SparseCellRef solves a plastic micro cell at n = 21 and 26 on the CPU, through the
load path e0 -> commit -> 1.5 e0 -> commit -> 0.5 e0 at the strain e0 = amp * default_rng(5).uniform(-1, 1, 6)
that TN.field((2, 2, 2), 5, amp, wobble=0) gives all eight macro Gauss points.  Every stage asserts
TN.check_conditions before anything is written.  A fixture holds settings and recorded results only (a few KB,
allow_pickle=False).  One stage takes about 20 s at n = 21 and 90 s at n = 26.

Run:  python tests/golden/make_micro_cells.py [--only NAME]                  (rewrites tests/golden/cell_*.npz)
      python tests/golden/make_micro_cells.py --sensitivity [--only NAME]    (prints; needs the fixtures)
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]

import test_gpu_micro_nl as TN  # noqa: E402
from micro_cell_sparse_ref import SparseCellRef  # noqa: E402

# the README's resolved-cell materials
MAT1, MAT2 = (1.0e7, 0.25, 7.6e3, 1.0e8), (1.0e8, 0.3, 1.0e9, 1.0e7)
SEED = 5
# name, type, n, the amplitudes in the order tried, whether stage 1.0 must have a partial yield front
FIXTURES = [
    ("cell_s21_a", 0, 21, (1.2e-3,), True),
    ("cell_s26_a", 0, 26, (4e-3,), False),
    ("cell_s26_b", 0, 26, (1.2e-3, 1.0e-3, 8e-4), True),
    ("cell_l21_a", 1, 21, (4e-3, 2e-3, 1.2e-3), False),
]
# the element whose phase --sensitivity inverts: a matrix element of the third element tile at n = 21, of
# the fourth (element 24, one element wide) at n = 26
SENSITIVITY = {"cell_s21_a": (17, 17, 3), "cell_l21_a": (17, 17, 3), "cell_s26_a": (24, 17, 17), "cell_s26_b": (24, 17, 17)}
PER_STAGE = ("sig", "C", "kappa", "its", "fmax", "margin", "mlin", "path", "nplastic")


def strain(amp):
    return amp * np.random.default_rng(SEED).uniform(-1, 1, 6)


def load_path(cell, amp, partial, stages=TN.STAGES):
    """the stages' results, or the reason this amplitude is not taken"""
    e0, hold, out = strain(amp), None, []
    for fac in stages:
        t0 = time.time()
        r = cell.point(fac * e0, hold)
        try:
            TN.check_conditions(r)
        except AssertionError as e:
            return None, f"stage {fac}: check_conditions {e}"
        if not r["path"]:
            return None, f"stage {fac}: below yield"
        print(f"    stage {fac}: newton {r['its']} margin {r['margin']:.2e} mlin {r['mlin']:.2e} kappa {r['kappa']:.2f} "
              f"nplastic {r['nplastic']} of {cell.matrix_points()} fmax {r['fmax']:.6e} {time.time() - t0:.0f} s", flush=True)
        if partial and fac == stages[0] and not 0 < r["nplastic"] < cell.matrix_points():
            return None, f"stage {fac}: no partial front"
        hold = r["h"]
        out.append(r)
    return out, None


def make(name, typ, n, amps, partial, write=True):
    t0 = time.time()
    cell = SparseCellRef(typ, n, MAT1, MAT2)
    print(f"{name}: type {typ} n {n}, kappa of the elastic K_ii {cell.kappa_lin:.2f}, {time.time() - t0:.0f} s", flush=True)
    for amp in amps:
        print(f"  amp {amp}", flush=True)
        rs, why = load_path(cell, amp, partial)
        if rs is not None:
            break
        print(f"  amp {amp} not taken: {why}", flush=True)
    else:
        print(f"{name}: no amplitude of {amps} meets the conditions; no fixture", flush=True)
        return None
    for r in rs:
        TN.check_conditions(r)
    fx = dict(typ=np.int64(typ), n=np.int64(n), mat1=np.array(MAT1), mat2=np.array(MAT2), seed=np.int64(SEED),
              amp=np.float64(amp), amps_tried=np.array(amps), e0=strain(amp), stages=np.array(TN.STAGES),
              Chom=cell.Chom, kappa_lin=np.float64(cell.kappa_lin), phase1=np.int64(cell.ph.sum()),
              matrix_points=np.int64(cell.matrix_points()))
    for k in PER_STAGE:
        fx[k] = np.array([r[k] for r in rs])
    if write:
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **fx)
        print(f"{name}: written, amp {amp}", flush=True)
    return fx


def sensitivity(name):
    """what one wrong element does: the phase of one matrix element inverted, stage 1.0 solved again, the
    change of sigma and C in units of the GPU tests' bar."""
    el = SENSITIVITY[name]
    fx = np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False)
    cell = SparseCellRef(int(fx["typ"]), int(fx["n"]), tuple(fx["mat1"]), tuple(fx["mat2"]), flip=[el])
    assert cell.matrix_points() == int(fx["matrix_points"]) - 8  # it was a matrix element
    r = cell.point(fx["e0"] * fx["stages"][0], None)
    bar = 100 * fx["kappa"][0] * TN.NL_RTOL
    ds = np.abs(r["sig"] - fx["sig"][0]).max() / np.abs(fx["sig"][0]).max()
    dc = np.abs(r["C"] - fx["C"][0]).max() / np.abs(fx["C"][0]).max()
    dh = np.abs(cell.Chom - fx["Chom"]).max() / np.abs(fx["Chom"]).max()
    hbar = 100 * fx["kappa_lin"] * 1e-12  # micro_rtol's default
    print(f"{name} with element {el} inverted, stage {fx['stages'][0]}: |d sigma| {ds:.3e} = {ds / bar:.3g} bars, "
          f"|d C| {dc:.3e} = {dc / bar:.3g} bars (bar {bar:.3e}); |d C_hom| {dh:.3e} = {dh / hbar:.3g} bars (bar {hbar:.3e})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", help="one fixture's name")
    ap.add_argument("--sensitivity", action="store_true")
    args = ap.parse_args()
    if args.sensitivity:
        for name in SENSITIVITY:
            if args.only in (None, name):
                sensitivity(name)
    else:
        for spec in FIXTURES:
            if args.only in (None, spec[0]):
                make(*spec)
