"""micro_nl_warm (-micro_nl_warm off|on), the checks that need no GPU: the flag parses
without a warning and touches no mcx_opts field, its word is checked with the flag named (code 2), the
new entry mcx_micro_nl_get_warm is exported, declared and refuses a null context, the ABI revision
stays 3, and a dense model of the rule itself.

The model (warm_solve) is CellRef's cell with the device's loop: the first state pass at the zero
interior gives D and the first norm, the predictor is u_w + sum_l (eps - eps_w)_l W_l in ascending l (the
elastic fields without a record), Newton stops at |D^-1 R| <= micro_nl_rtol |D^-1 R_0|, every linear
solve is a Jacobi-PCG (D of the first pass) that stops at |D^-1 r| <= micro_rtol norm0, and tangent
column l starts from W_l with norm0 taken from the zero start.  It counts the PCG iterations.  The
claims: the results stay within the bar of the 1e-13 reference (100 kappa micro_nl_rtol of the largest
entry) and the warm start takes strictly fewer PCG iterations than the elastic start.

mcx_apply_args and the getter's round trip need a context, so a device: tests/test_gpu_micro_nl_warm.py."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import macroc_amd as M
import test_gpu_micro_nl as TN
import test_gpu_micro_nl_global as TGL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NL_RTOL, CG_RTOL = 1e-10, 1e-12  # micro_nl_rtol's and micro_rtol's defaults


# ---------------------------------------------------------------- the flag and the entry point
@pytest.mark.parametrize("flags", [["-micro_nl_warm", "off"], ["-micro_nl_warm", "on"],
                                   ["-micro_nl_solver", "grid", "-micro_nl_tangent", "block", "-micro_nl_apply", "fused",
                                    "-micro_nl_warm", "on", "-micro_nl_ls", "5"]])
def test_flag_parses_without_a_warning(flags, capfd):
    base = M.parse_args([])
    capfd.readouterr()
    o = M.parse_args(flags)
    assert capfd.readouterr().err == ""
    for f, _ in M.Opts._fields_:  # the flag's value touches no mcx_opts field
        a, b = getattr(o, f), getattr(base, f)
        assert (list(a) == list(b)) if hasattr(a, "__len__") else (a == b), f
    o = M.parse_args(["-mat_law", "micro_nl", "-micro_n", "12", *flags, "-micro_type", "0"])
    assert capfd.readouterr().err == ""
    assert o.micro_n == 12 and o.micro_type == 0 and o.mat_law == M.parse_args(["-mat_law", "micro_nl"]).mat_law


@pytest.mark.parametrize("law", ["elastic", "plastic", "micro"])
def test_other_laws_accept_the_flag(law, capfd):
    capfd.readouterr()
    o = M.parse_args(["-mat_law", law, "-micro_nl_warm", "on"])
    assert capfd.readouterr().err == ""
    assert o.mat_law == M.parse_args(["-mat_law", law]).mat_law


def test_near_misses_are_still_reported(capfd):
    capfd.readouterr()
    M.parse_args(["-micro_nl_warms", "on"])
    assert "-micro_nl_warms" in capfd.readouterr().err


@pytest.mark.parametrize("bad", ["1", "On", "warm", "elastic"])
def test_word_is_checked_with_code_2(bad):
    with pytest.raises(M.MacrocError, match="-micro_nl_warm: off or on, got " + bad + "$"):
        M.parse_args(["-micro_nl_warm", bad])
    argv = (C.c_char_p * 2)(b"-micro_nl_warm", bad.encode())
    o = M.Opts()
    M.lib().mcx_default_opts(C.byref(o))
    assert M.lib().mcx_parse_args(C.byref(o), 2, argv) == 2
    assert M.lib().mcx_last_error().decode() == "-micro_nl_warm: off or on, got " + bad


def test_entry_is_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "macroc_amd.h")).read()
    assert "mcx_micro_nl_get_warm" in M.EXPORTS and hasattr(M.lib(), "mcx_micro_nl_get_warm")
    assert re.search(r"\bint\s+mcx_micro_nl_get_warm\s*\(void\* ctx, int\* option, int\* used\);", hdr)
    for word in ('"micro_nl_warm"', "-micro_nl_warm off|on"):
        assert word in hdr, word
    declared = set(re.findall(r"\b(mcx_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(M.EXPORTS) and len(M.EXPORTS) == len(declared)
    assert hasattr(M.Macroc, "micro_nl_warm")
    assert M.lib().mcx_abi_version() == 3 == M.ABI_VERSION


def test_entry_refuses_a_null_context():
    opt, used = C.c_int(7), (C.c_int * 8)(*([9] * 8))
    assert M.lib().mcx_micro_nl_get_warm(None, C.byref(opt), used) == 1
    assert opt.value == 7 and list(used) == [9] * 8
    assert "null context" in M.lib().mcx_last_error().decode()


def test_readme_design_and_driver_list_the_flag():
    assert "-micro_nl_warm" in open(os.path.join(ROOT, "README.md")).read()
    assert "-micro_nl_warm" in open(os.path.join(ROOT, "macroc_amd", "driver", "main.c")).read()
    assert "micro_nl_warm" in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---------------------------------------------------------------- the dense model of the rule
def pcg(K, b, x0, dinv, norm0, rtol, max_it, warm=False):
    """Jacobi-PCG from x0 with the device's stop |D^-1 r| <= rtol norm0; (x, iterations).  warm: the
    stop is also tested before the first iteration (x0 = 0 has |D^-1 r| = norm0 there)."""
    x = x0.copy()
    r = b - K @ x
    z = dinv * r
    if warm and np.linalg.norm(z) <= rtol * norm0:
        return x, 0
    p, rz = z.copy(), r @ z
    for it in range(1, max_it + 1):
        q = K @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        z = dinv * r
        if np.linalg.norm(z) / norm0 <= rtol:
            return x, it
        rz, beta = r @ z, (r @ z) / rz
        p = z + beta * p
    raise AssertionError("the PCG did not converge")


def warm_solve(ref, eps, hold, rec=None, start=1, nl_rtol=NL_RTOL, rtol=CG_RTOL, nl_max_it=20):
    """one cell solve by the rule of DESIGN §22.  rec: the warm record (u, W [ndof][6], eps) or None,
    then the point follows micro_nl_start = start.  Returns sigma, C, the new history, the Newton steps,
    the PCG iterations of Newton and of the six columns, and the new record."""
    fr = ~ref.bd
    max_it = 10 * int(fr.sum())
    u = ref.boundary_field(eps)

    def state(u):
        s, hn, f, sn, Ct = ref.j2(ref.strains(u), hold)
        R = np.zeros(len(u))
        np.add.at(R, ref.edof, np.einsum("gki,egk->ei", ref.B, s) * ref.detJ)
        return s, hn, f, Ct, R

    s, hn, f, Ct, R = state(u)  # the first state pass: at the zero interior, whatever follows
    dinv = 1.0 / np.diag(ref.stiffness(Ct)[np.ix_(fr, fr)])
    n0 = np.linalg.norm(dinv * R[fr])
    if n0 != 0.0 and (rec is not None or start):
        if rec is not None:
            pred = rec["u"].copy()
            for l in range(6):  # ascending l
                pred += (eps[l] - rec["eps"][l]) * rec["W"][:, l]
        else:
            W0 = TGL.unit_fields(ref)
            pred = np.zeros(len(u))
            for l in range(6):
                pred += eps[l] * W0[:, l]
        u[fr] = pred[fr]
        s, hn, f, Ct, R = state(u)
    steps, cg_newton = 0, 0
    while True:
        nrm = np.linalg.norm(dinv * R[fr])
        if n0 == 0.0 or nrm <= nl_rtol * n0:
            break
        assert steps < nl_max_it, "Newton gave up"
        Kii = ref.stiffness(Ct)[np.ix_(fr, fr)]
        dx, its = pcg(Kii, -R[fr], np.zeros(int(fr.sum())), dinv, nrm, rtol, max_it)
        cg_newton += its
        steps += 1
        u[fr] += dx
        s, hn, f, Ct, R = state(u)
    Kt = ref.stiffness(Ct)
    Kii, Kib = Kt[np.ix_(fr, fr)], Kt[np.ix_(fr, ~fr)]
    W, Cm, cg_cols = np.zeros((len(u), 6)), np.zeros((6, 6)), []
    for l in range(6):
        e = np.zeros(6)
        e[l] = 1.0
        W[:, l] = ref.boundary_field(e)
        b = -Kib @ W[~fr, l]
        norm0 = np.linalg.norm(dinv * b)  # the zero start's, also under a warm start
        its = 0
        if norm0 != 0.0:
            x0 = rec["W"][fr, l] if rec is not None else np.zeros(int(fr.sum()))
            W[fr, l], its = pcg(Kii, b, x0, dinv, norm0, rtol, max_it, warm=rec is not None)
        cg_cols.append(its)
        Cm[:, l] = np.einsum("egkl,egl->k", Ct, ref.strains(W[:, l])) * ref.detJ
    return dict(sig=s.sum((0, 1)) * ref.detJ, C=0.5 * (Cm + Cm.T), h=hn, steps=steps, cg_newton=cg_newton,
                cg_cols=cg_cols, cg=cg_newton + sum(cg_cols), rec=dict(u=u.copy(), W=W, eps=np.array(eps, float)))


@functools.lru_cache(maxsize=None)
def scenario(typ, n):
    """load (5, 4e-3): the point is solved at e0 (no record), then asked again at e0, at (1 + 1e-3) e0,
    and, after a commit, at 1.5 e0: each time from the record of the solve at e0 and, for comparison,
    from the elastic start; the 1e-13 reference of each."""
    ref = TN.cell(typ, n)
    e0 = 4e-3 * np.random.default_rng(5).uniform(-1, 1, 6)
    first = warm_solve(ref, e0, ref.zero_hist)
    again = warm_solve(ref, e0, ref.zero_hist)
    for k in ("sig", "C", "h"):  # without a record the rule is micro_nl_start's: the same bits twice
        assert np.array_equal(first[k], again[k])
    cases = {}
    for name, eps, hold in (("same", e0, ref.zero_hist), ("near", (1 + 1e-3) * e0, ref.zero_hist),
                            ("commit", 1.5 * e0, first["h"])):
        cases[name] = dict(warm=warm_solve(ref, eps, hold, rec=first["rec"]), elastic=warm_solve(ref, eps, hold),
                           ref=ref.solve(eps, hold))
    return first, cases


@pytest.mark.parametrize("typ,n", [(0, 5), (1, 4)])
def test_dense_model_of_the_rule(typ, n):
    first, cases = scenario(typ, n)
    assert first["steps"] > 0 and first["cg_newton"] > 0 and min(first["cg_cols"]) > 0  # the load yields: CGs ran
    for name, c in cases.items():
        r, w, e = c["ref"], c["warm"], c["elastic"]
        assert r["its"] <= 10 and r["margin"] >= TN.MARGIN
        bar = 100 * r["kappa"] * NL_RTOL
        for run, x in (("warm", w), ("elastic", e)):
            es = np.abs(x["sig"] - r["sig"]).max() / np.abs(r["sig"]).max()
            ec = np.abs(x["C"] - r["C"]).max() / np.abs(r["C"]).max()
            print(f"cell ({typ},{n}) {name} {run}: newton {x['steps']} / cg {x['cg_newton']} + {sum(x['cg_cols'])} "
                  f"{x['cg_cols']} err sigma {es:.2e} C {ec:.2e} bar {bar:.2e}")
            assert es <= bar and ec <= bar
        assert w["cg"] < e["cg"], (name, w["cg"], e["cg"])
        assert w["steps"] <= e["steps"]
    assert cases["same"]["warm"]["steps"] == 0  # the record solves the same strain: the predictor converges
