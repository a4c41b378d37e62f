"""micro_nl_warm (-micro_nl_warm off|on): micro_nl_solver 1 starts a slotted point's Newton
loop and its six tangent columns from the slot's warm record, the last converged field, columns and
strain.  What is pinned here:

1. a point without a valid record follows micro_nl_start bit for bit (the first call of a context);
2. a repeat at the same u is solved by the predictor (0 Newton steps) in fewer CG iterations, within the
   bar of the dense reference (TN.CellRef: 100 kappa micro_nl_rtol of the largest entry);
3. the load path 1.0 -> commit -> 1.5 -> commit -> 0.5, every stage evaluated twice (u, then
   (1 + 1e-3) u), stays within the bar, and the second evaluations take fewer CG iterations;
4. block / seq, fused / split, the poll interval, the batch, the macro grid and a second run give the
   same bits under the option;
5. a failed solve leaves the record invalid; 6. switching and the store's bytes; 7. the cases without
   effect; 8. with micro_nl_ls; 9. the driver.

The cells are the smallest that reach every path: sphere n = 9 and 10 (two tiles per axis), a layer n = 9,
a layer n = 3 (one interior node), n = 2 (none) and one sphere n = 17 (three tiles per axis)."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import macroc_amd as M
import test_gpu_micro_nl as TN
import test_gpu_micro_nl_grid as TG
import test_gpu_micro_nl_global as TGL
import test_gpu_micro_nl_block as TB

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NL_RTOL = TN.NL_RTOL
CELLS = [(0, 9), (0, 10), (1, 9), (1, 3), (1, 2)]
NEAR = 1 + 1e-3
KEYS = TB.KEYS


def record_bytes(n):
    """the documented size of a slot's warm record: seven fields of 3 n^3 doubles and a 64-byte header"""
    return 7 * 24 * n ** 3 + 64


def snap(m, u):
    eps, sig, Cg, info = TN.evaluate(m, u)
    return dict(eps=eps, sig=sig, C=Cg, f=np.array(m.nonlinear_stats()[1]), path=info["path"],
                newton_its=info["newton_its"], cg_its=info["cg_its"], rnorm=info["rnorm"], cols=m.micro_nl_tangent_its(),
                steps=m.micro_nl_steps(), warm=m.micro_nl_warm(), slots=info["slots"], dev=m.get_info()["device_bytes"])


def run_path(typ, n, warm, tangent=0, apply=0, u1=None, grid=(2, 2, 2), stages=TN.STAGES, facs=(1.0, NEAR), **opts):
    """every stage evaluated at fac x stage x u1 for the facs in turn, then committed"""
    u1 = TB.load() if u1 is None else u1
    out = []
    with TG.grid_ctx(TN.nl_argv(typ, n, grid), micro_nl_tangent=tangent, micro_nl_apply=apply, micro_nl_warm=warm,
                     **opts) as m:
        assert m.micro_nl_warm_option() == warm
        for st in stages:
            for fac in facs:
                out.append(snap(m, fac * st * u1))
            m.update_vars()
    return out


@functools.lru_cache(maxsize=None)
def cell_path(typ, n, warm, tangent=0, apply=0, start=0, stages=TN.STAGES, wobble=True):
    u1 = TB.load() if wobble else TN.field((2, 2, 2), 5, 4e-3, wobble=0)
    return run_path(typ, n, warm, tangent, apply, u1=u1, stages=stages, micro_nl_start=start)


def same_bits(a, b, sel=None, cols=False, warm=True):
    assert len(a) == len(b)
    TB.same_bits(a, b, sel)
    for x, y in zip(a, b):
        pick = (lambda v: v) if sel is None else (lambda v: v[sel])
        for k in ("ls_rejects", "min_step"):
            assert np.array_equal(x["steps"][k], pick(y["steps"][k])), k
        if warm:
            assert np.array_equal(x["warm"], pick(y["warm"]))
        if cols:
            assert np.array_equal(x["cols"], pick(y["cols"]))


def solved(r):
    return r["path"].astype(bool)


# ---------------------------------------------------------------- 1. the first call: the fallback
@pytest.mark.parametrize("start", [0, 1])
@pytest.mark.parametrize("typ,n", CELLS)
def test_first_call_follows_micro_nl_start(typ, n, start):
    off, on = (run_path(typ, n, w, stages=(1.0,), facs=(1.0,), micro_nl_start=start) for w in (0, 1))
    same_bits(off, on, warm=False)
    assert off[0]["path"].any()
    assert not off[0]["warm"][~solved(off[0])].any() and not on[0]["warm"][~solved(on[0])].any()
    want = 0 if n == 2 else 1  # n = 2 has no interior dof: nothing is solved, nothing kept
    assert (off[0]["warm"][solved(off[0])] == want).all() and (on[0]["warm"][solved(on[0])] == want).all()


# ---------------------------------------------------------------- 2., 3. against the dense reference
@functools.lru_cache(maxsize=None)
def reference_path(typ, n, wobble):
    """the reference through cell_path's evaluations, fed the strains the device reports; one strain per
    evaluation without the wobble (the eight points are then the same problem)"""
    ref, runs = TN.cell(typ, n), cell_path(typ, n, 1, start=1, wobble=wobble)
    hold, out = [None] * 8, []
    for k, y in enumerate(runs):
        rs = []
        for q in range(8):
            if not wobble and q > 0:
                assert np.abs(y["eps"][q] - y["eps"][0]).max() <= 1e-15  # the same strain but for its last bits
                rs.append(rs[0])
                continue
            rs.append(ref.point(y["eps"][q], hold[q]))
        out.append(rs)
        if k % 2 == 1:  # the commit follows the stage's second evaluation
            hold = [r["h"] if r["path"] else h for r, h in zip(rs, hold)]
    return out


def check_against(y, rs, what):
    worst = 0.0
    for q in range(8):
        r = rs[q]
        TN.check_conditions(r)
        assert y["path"][q] == r["path"]
        bar = 100 * r["kappa"] * NL_RTOL
        es = np.abs(y["sig"][q] - r["sig"]).max() / np.abs(r["sig"]).max()
        ec = np.abs(y["C"][q] - r["C"]).max() / np.abs(r["C"]).max()
        worst = max(worst, es / bar, ec / bar)
        assert es <= bar and ec <= bar, (what, q, es, ec, bar)
        assert y["rnorm"][q] <= NL_RTOL and np.array_equal(y["C"][q], y["C"][q].T)
    fref, smax = max(r["fmax"] for r in rs), max(np.abs(r["sig"]).max() for r in rs)
    ef = abs(float(y["f"]) - fref) / smax
    bar = 100 * max(r["kappa"] for r in rs) * NL_RTOL
    print(f"{what}: worst error / bar {worst:.2e}, f_trial error {ef:.2e} bar {bar:.2e}; newton {y['newton_its'].tolist()} "
          f"cg {y['cg_its'].tolist()} warm {y['warm'].tolist()}")
    assert ef <= bar


def test_repeat_at_the_same_u():
    """sphere n = 9: the second homogenize at the same u starts every point from its record, the
    predictor meets the Newton stop, and the columns take fewer iterations than from zero"""
    u1 = TN.field((2, 2, 2), 5, 4e-3, wobble=0)  # one strain: one dense solve judges the eight points
    out = {}
    for w in (0, 1):
        with TG.grid_ctx(TN.nl_argv(0, 9), micro_nl_warm=w) as m:
            out[w] = [snap(m, u1), snap(m, u1)]
    off, on = out[0], out[1]
    same_bits(off[:1], on[:1], warm=False)
    same_bits(off[:1], off[1:], warm=False)  # without the option the repeat is the first call again
    s = solved(on[1])
    assert s.all() and (on[0]["warm"] == 1).all() and (on[1]["warm"] == 2).all() and (off[1]["warm"] == 1).all()
    assert not on[1]["newton_its"].any()
    print("repeat at the same u, sphere n = 9: cg off", off[1]["cg_its"].tolist(), "on", on[1]["cg_its"].tolist(),
          "ratio %.3f" % (on[1]["cg_its"].sum() / off[1]["cg_its"].sum()))
    assert on[1]["cg_its"].sum() < off[1]["cg_its"].sum()
    assert np.abs(on[1]["eps"] - on[1]["eps"][0]).max() <= 1e-15  # the same strain but for its last bits
    check_against(on[1], [TN.cell(0, 9).point(on[1]["eps"][0], None)] * 8, "repeat")


@pytest.mark.parametrize("typ,n,wobble", [(0, 9, False), (1, 9, False), (1, 3, True)])
def test_load_path_against_the_reference(typ, n, wobble):
    """1.0 -> commit -> 1.5 -> commit -> 0.5, each stage at u and at (1 + 1e-3) u, under micro_nl_start 1 (plain
    Newton gives up on the unload of soft cells), the option on against off"""
    on, off = cell_path(typ, n, 1, start=1, wobble=wobble), cell_path(typ, n, 0, start=1, wobble=wobble)
    refs = reference_path(typ, n, wobble)
    assert len(on) == len(off) == len(refs) == 6
    for k, (x, y, rs) in enumerate(zip(off, on, refs)):
        assert np.array_equal(x["eps"], y["eps"]) and np.array_equal(x["path"], y["path"])
        check_against(y, rs, f"cell ({typ},{n}) evaluation {k} on")
        check_against(x, rs, f"cell ({typ},{n}) evaluation {k} off")
        s = solved(y)
        if k % 2 == 1:  # the second evaluation of a stage: from the record of the first
            assert s.any() and (y["warm"][s] == 2).all()
            print(f"cell ({typ},{n}) stage {k // 2} second evaluation: cg off {x['cg_its'].sum()} on {y['cg_its'].sum()} "
                  f"ratio {y['cg_its'].sum() / x['cg_its'].sum():.3f} newton off {x['newton_its'].max()} on {y['newton_its'].max()}")
            assert y["cg_its"].sum() < x["cg_its"].sum()
        assert (x["warm"][solved(x)] == 1).all()
    assert (on[0]["warm"][solved(on[0])] == 1).all()  # a fresh context has no record


# ---------------------------------------------------------------- 4. settings that must not change bits
@pytest.mark.parametrize("typ,n", [(0, 9), (0, 10), (1, 9), (1, 3)])
def test_block_and_fused_give_the_same_bits_under_the_option(typ, n):
    base = cell_path(typ, n, 1, 0, 0, stages=(1.0, 0.5))
    assert any((r["warm"] == 2).any() for r in base)
    for tangent, apply in ((0, 1), (1, 0), (1, 1)):
        same_bits(base, cell_path(typ, n, 1, tangent, apply, stages=(1.0, 0.5)))
    same_bits(cell_path(typ, n, 1, 1, 0, stages=(1.0, 0.5)), cell_path(typ, n, 1, 1, 1, stages=(1.0, 0.5)), cols=True)
    for k, y in enumerate(cell_path(typ, n, 1, 1, 1, stages=(1.0, 0.5))):
        print(f"cell ({typ},{n}) evaluation {k}: warm {y['warm'].tolist()} newton {y['newton_its'].tolist()} columns "
              f"{y['cols'].tolist()}")


@functools.lru_cache(maxsize=None)
def base_n10():
    return run_path(0, 10, 1, stages=(1.0,))


@pytest.mark.parametrize("poll,blocks,big,tangent", [(1, 0, False, 0), (7, 0, False, 1), (16, 0, False, 0), (16, 3, False, 1),
                                                     (16, 0, True, 0), (7, 3, True, 1)])
def test_bits_do_not_depend_on_poll_batch_slot_or_grid(poll, blocks, big, tangent):
    base = base_n10()
    assert (base[1]["warm"] == 2).all() and base[1]["cg_its"].sum() < base[0]["cg_its"].sum()
    if big:
        out = run_path(0, 10, 1, tangent, 1, u1=TB.embedded(TB.load()), grid=(3, 2, 2), stages=(1.0,), micro_grid_poll=poll,
                       micro_mem_blocks=blocks)
        assert out[0]["path"][:8].all()  # the first element is solved too
        same_bits(base, out, slice(8, None))
    else:
        out = run_path(0, 10, 1, tangent, 1, stages=(1.0,), micro_grid_poll=poll, micro_mem_blocks=blocks)
        same_bits(base, out)


def test_two_runs_are_bitwise_equal():
    same_bits(base_n10(), run_path(0, 10, 1, stages=(1.0,)))


def test_three_tiles_per_axis():
    """sphere n = 17, block + fused against seq + split: the first call and the repeat at (1 + 1e-3) u"""
    a, b = (run_path(0, 17, 1, t, f, stages=(1.0,)) for t, f in ((0, 0), (1, 1)))
    same_bits(a, b)
    assert a[0]["path"].all() and (a[0]["warm"] == 1).all() and (a[1]["warm"] == 2).all()
    assert (a[1]["rnorm"] <= NL_RTOL).all()
    print("n = 17: newton", a[0]["newton_its"].max(), "->", a[1]["newton_its"].max(), "cg", a[0]["cg_its"].sum(), "->",
          a[1]["cg_its"].sum())
    assert a[1]["cg_its"].sum() < a[0]["cg_its"].sum()


# ---------------------------------------------------------------- 5. failures
def test_a_failed_solve_leaves_the_record_invalid():
    u1 = TB.load()
    first = run_path(0, 5, 0, stages=(1.0,), facs=(1.0,))[0]  # test 1's first call
    with TG.grid_ctx(TN.nl_argv(0, 5), micro_nl_warm=1, micro_max_it=3) as m:
        m.set_u(u1)
        m.set_strains()
        with pytest.raises(M.MacrocError, match=r"failed \(33\): -mat_law micro: the micro cell's CG did not converge "
                                                r"for load case 0 \(unit strain component xx\): 3 iterations"):
            m.homogenize()
        m.set_option("micro_max_it", 0)  # back at the default: the same context goes on
        a = snap(m, u1)
        same_bits([first], [a], warm=False)
        assert (a["warm"] == 1).all()
        b = snap(m, u1)
        assert (b["warm"] == 2).all() and not b["newton_its"].any() and b["cg_its"].sum() < a["cg_its"].sum()
        # every cell solve fails (a Newton stop that cannot be met, one step allowed): today's code and message
        m.set_option("micro_nl_rtol", 1e-300)
        m.set_option("micro_nl_max_it", 1)
        with pytest.raises(M.MacrocError, match=r"failed \(35\): .*8 of 8 micro cells did not converge; worst: Gauss "
                                                r"point \d+ \(Newton gave up\): 1 Newton iterations"):
            m.homogenize()
        m.set_option("micro_nl_rtol", NL_RTOL)
        m.set_option("micro_nl_max_it", 20)
        c = snap(m, u1)  # the records were invalidated: the first call's bits
        same_bits([first], [c], warm=False)
        assert (c["warm"] == 1).all()
        d = snap(m, u1)  # and it warms up again
        same_bits([b], [d])


# ---------------------------------------------------------------- 6. switching
def test_switching_and_the_store():
    n, u1 = 5, TB.load()
    with TG.grid_ctx(TN.nl_argv(0, n)) as m:
        a = snap(m, u1)
        assert a["path"].all() and a["slots"] >= 8 and (a["warm"] == 1).all()
        m.set_option("micro_nl_warm", 1)  # with slots in use: the records start invalid
        b = snap(m, u1)
        same_bits([a], [b])
        assert b["dev"] == a["dev"] + b["slots"] * record_bytes(n) and b["slots"] == a["slots"]
        c = snap(m, u1)
        assert (c["warm"] == 2).all() and c["dev"] == b["dev"] and c["cg_its"].sum() < b["cg_its"].sum()
        m.update_vars()  # the commit does not touch the records
        d = snap(m, u1)
        assert (d["warm"] == 2).all() and d["dev"] == b["dev"]
        m.set_option("micro_nl_warm", 0)  # releases the store
        assert m.get_info()["device_bytes"] == a["dev"] and m.micro_nl_warm_option() == 0
        e = snap(m, u1)
        assert (e["warm"] == 1).all() and e["dev"] == a["dev"]
        m.set_option("micro_nl_warm", 1)  # and on again: invalid records, the bits of the option-off call
        f = snap(m, u1)
        same_bits([e], [f])
        assert f["dev"] == b["dev"]
        assert (snap(m, u1)["warm"] == 2).all()
        m.set_option("micro_nl_slots", f["slots"] + 4)  # the pool moves; the records are invalidated
        g = snap(m, u1)
        same_bits([e], [g])
        assert g["slots"] == f["slots"] + 4
        assert g["dev"] == f["dev"] + 4 * (m.micro_nl_info()["bytes_per_slot"] + record_bytes(n))


# ---------------------------------------------------------------- 7. the cases without effect
@pytest.mark.parametrize("mem", [0, 1])
def test_solver_0_takes_the_option_without_effect(mem):
    u1, out = TB.load(), []
    for w in (0, 1):
        with M.Macroc(TN.nl_argv(0, 4)) as m:
            m.set_option("micro_mem", mem)
            m.set_option("micro_nl_warm", w)
            out.append([snap(m, u1), snap(m, NEAR * u1)])
            assert m.micro_nl_warm_option() == w
    same_bits(out[0], out[1])
    for r in out[1]:
        assert r["path"].all() and (r["warm"] == 1).all()
    assert out[0][1]["dev"] == out[1][1]["dev"]


def test_below_yield_there_is_no_store():
    grid = (5, 4, 3)
    u = TN.field(grid, 11, 2e-5)
    dev = []
    for w in (0, 1):
        with TG.grid_ctx(TN.nl_argv(1, 9, grid), micro_nl_warm=w) as a:
            ba, va = TN.assemble(a, u)
            sa, info = a.stress(), a.micro_nl_info()
            assert not info["path"].any() and info["slots"] == 0 and info["slots_used"] == 0
            assert not a.micro_nl_warm().any()
            dev.append(a.get_info()["device_bytes"])
    assert dev[0] == dev[1]
    with M.Macroc(TN.nl_argv(1, 9, grid, law="micro", extra=("-micro_solver", "grid"))) as b:
        bb, vb = TN.assemble(b, u)
        sb = b.stress()
    assert np.linalg.norm(bb) > 0
    assert np.array_equal(sa, sb) and np.array_equal(ba, bb) and np.array_equal(va, vb)


def test_n2_is_untouched():
    off, on = (run_path(1, 2, w, stages=(1.0, 1.5)) for w in (0, 1))
    same_bits(off, on)
    for r in on:
        assert r["path"].all() and not r["warm"].any() and not r["cg_its"].any()
    assert off[-1]["dev"] == on[-1]["dev"]


def test_option_values_and_words():
    u1 = TB.load()
    with TG.grid_ctx(TN.nl_argv(0, 4)) as m:
        assert m.micro_nl_warm_option() == 0
        for bad in (2, -1, 0.5):
            with pytest.raises(M.MacrocError, match=r"micro_nl_warm: 0 \(off.*\) or 1 \(on.*\)"):
                m.set_option("micro_nl_warm", bad)
            assert M.lib().mcx_set_option(m._ctx, b"micro_nl_warm", float(bad)) == 1
        assert m.micro_nl_warm_option() == 0
        sig0 = snap(m, u1)["sig"]
    for law in ("elastic", "plastic", "micro"):  # the other laws accept the option without effect
        with M.Macroc(TN.nl_argv(0, 4, law=law)) as m:
            m.set_option("micro_nl_warm", 1)
            assert m.micro_nl_warm_option() == 1 and not m.micro_nl_warm().any()
    for where in (M.parse_args, M.Macroc):
        with pytest.raises(M.MacrocError, match="-micro_nl_warm: off or on, got grid"):
            where(TN.nl_argv(0, 4, extra=("-micro_nl_warm", "grid")))
    for word, value in (("off", 0), ("on", 1)):  # the flag is the option (mcx_apply_args)
        with M.Macroc(TN.nl_argv(0, 4, extra=("-micro_nl_solver", "grid", "-micro_nl_warm", word))) as m:
            assert m.micro_nl_warm_option() == value
            assert np.array_equal(snap(m, u1)["sig"], sig0)
            assert (snap(m, u1)["warm"] == 1 + value).all()


# ---------------------------------------------------------------- 8. with the line search
@pytest.mark.slow
def test_line_search_with_the_option():
    """DESIGN §19's sphere cell (n = 12, one strain, e0 -> commit -> 1.25 e0) with micro_nl_ls 5 and the option
    on: the second stage starts from the record of the first and converges to the reference's result"""
    n, u1 = TGL.SPHERE_N, TN.field((2, 2, 2), 5, 4e-3, wobble=0)
    ref = TN.cell(0, n)
    e0 = 4e-3 * np.random.default_rng(5).uniform(-1, 1, 6)
    r1 = TGL.solve_global(ref, e0, ref.zero_hist, 1, 5, kappa=False)
    r2 = TGL.solve_global(ref, 1.25 * e0, r1["h"], 1, 5)
    assert r1["status"] == 0 and r2["status"] == 0
    b = run_path(0, n, 1, u1=u1, stages=(1.0, 1.25), facs=(1.0,), micro_nl_ls=5, micro_nl_start=1)
    y, bar = b[1], 100 * r2["kappa"] * NL_RTOL
    assert np.abs(y["eps"] - 1.25 * e0).max() <= 1e-15
    es = np.abs(y["sig"] - r2["sig"]).max() / np.abs(r2["sig"]).max()
    ec = np.abs(y["C"] - r2["C"]).max() / np.abs(r2["C"]).max()
    print(f"sphere n {n} ls 5 warm: kappa {r2['kappa']:.1f} err sigma {es:.2e} C {ec:.2e} bar {bar:.2e} newton "
          f"{y['newton_its'].tolist()} ref {r2['its']} rejects {y['steps']['ls_rejects'].tolist()} ref {r2['rejects']} "
          f"smallest step {y['steps']['min_step'].tolist()} cg {y['cg_its'].tolist()} (first stage {b[0]['cg_its'].tolist()})")
    assert (b[0]["warm"] == 1).all() and (y["warm"] == 2).all()
    assert y["path"].all() and (y["rnorm"] <= NL_RTOL).all()
    assert es <= bar and ec <= bar


# ---------------------------------------------------------------- 9. the driver
def test_driver_takes_the_flag(tmp_path):
    """the README's -micro_nl_solver grid command at -micro_n 10 runs to the end with -micro_nl_warm on; the macro
    Newton residuals agree with the unflagged run's within the bar (of the time step's first residual) and the
    seven printed digits"""
    exe = os.path.join(ROOT, "macroc_amd", "driver", "macroc_amd")
    argv = [exe, "-da_grid_x", "4", "-da_grid_y", "4", "-da_grid_z", "4", "-ts", "2", "-mat_law", "micro_nl",
            "-micro_n", "10", "-micro_nl_solver", "grid", "-micro_type", "0", "-micro_mat_1", "1e7,0.25,7.6e3,1e8",
            "-micro_mat_2", "1e8,0.3,1e9,1e7"]
    res = {}
    for word in ("off", "on"):
        d = tmp_path / word
        d.mkdir()
        out = subprocess.run(argv + ["-micro_nl_warm", word], cwd=d, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "options you set that were not used" not in out.stderr and "has no effect" not in out.stderr
        assert "Elapsed time" in out.stdout
        res[word] = [float(x) for x in re.findall(r"^\|RES\| = (\S+)$", out.stdout, re.M)]
        counts = [int(l.split(":")[1].split()[0]) for l in out.stdout.splitlines() if l.startswith("Non-Linear Gauss points : ")]
        assert counts and max(counts) > 0, out.stdout
    bar = 100 * TG.scaled_kappa(10) * NL_RTOL
    print("driver |RES| off", res["off"], "on", res["on"])
    assert len(res["off"]) == len(res["on"]) > 2
    top = max(res["off"])
    for a, b in zip(res["off"], res["on"]):
        assert abs(a - b) <= bar * top + 1e-6 * max(a, b), (a, b)
