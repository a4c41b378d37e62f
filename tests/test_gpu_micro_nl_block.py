"""Option micro_nl_tangent 1 (-micro_nl_tangent block): micro_nl_solver 1 advances the six
frozen-K_T tangent solves of a solved point together, column l with its own vectors, sums and CG
record.  Every column keeps the sequential solve's products and summation order, so the option
changes no bit: the tests compare `block` with `seq` by np.array_equal, never by a tolerance.

The materials and the load are test_gpu_micro_nl_grid's (TN.MAT1 / TN.MAT2, load (5, 4e-3) through
1.0 -> commit -> 1.5 -> commit -> 0.5), on which the law's plain Newton converges.  A run is made once
per (cell, setting) and shared.

Not executed by any test: a tangent column that ends unconverged (k_mnlb_scalar<1> / <2> setting the
column's status, k_mnlb_scalar<0> failing the point without writing the tangent).  micro_max_it bounds
every CG of the cell, so a limit that stops a column stops C_hom's or Newton's CG first; that branch is
covered by reading the code only.  There the reported CG count holds all six columns' iterations, where
the sequential columns stop at the first that fails: only a failed point's count differs.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import macroc_amd as M
import test_gpu_micro_nl as TN
import test_gpu_micro_nl_grid as TG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# sphere n = 9: one full tile; sphere n = 10: two tiles per axis, partial ones; a layer; one interior node; none
CELLS = [(0, 9), (0, 10), (1, 9), (1, 3), (1, 2)]
KEYS = ("eps", "sig", "C", "f", "path", "newton_its", "cg_its", "rnorm")


def load(grid=(2, 2, 2)):
    return TN.field(grid, 5, 4e-3)


def run_stages(typ, n, tangent, u1=None, grid=(2, 2, 2), stages=TN.STAGES, **opts):
    u1 = load() if u1 is None else u1
    out = []
    with TG.grid_ctx(TN.nl_argv(typ, n, grid), micro_nl_tangent=tangent, **opts) as m:
        assert m.micro_nl_tangent() == tangent
        for fac in stages:
            eps, sig, Cg, info = TN.evaluate(m, fac * u1)
            out.append(dict(eps=eps, sig=sig, C=Cg, f=np.array(m.nonlinear_stats()[1]), path=info["path"],
                            newton_its=info["newton_its"], cg_its=info["cg_its"], rnorm=info["rnorm"],
                            cols=m.micro_nl_tangent_its(), steps=m.micro_nl_steps()))
            m.update_vars()
    return out


@functools.lru_cache(maxsize=None)
def cell_run(typ, n, tangent):
    return run_stages(typ, n, tangent)


def same_bits(a, b, sel=None):
    """every result of a equals b's (sel: the Gauss points of b to compare; f, the largest trial f of
    all points, only without a selection)"""
    for x, y in zip(a, b):
        for k in KEYS:
            if k == "f":
                assert sel is not None or np.array_equal(x[k], y[k]), k
            else:
                assert np.array_equal(x[k], y[k] if sel is None else y[k][sel]), k


# ---------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("typ,n", CELLS)
def test_block_gives_the_sequential_bits(typ, n):
    seq, blk = cell_run(typ, n, 0), cell_run(typ, n, 1)
    assert len(seq) == len(blk) == 3
    same_bits(seq, blk)
    for st, (x, y) in enumerate(zip(seq, blk)):
        print(f"cell ({typ},{n}) stage {st}: newton {y['newton_its']} cg {y['cg_its']} columns {y['cols'].tolist()}")
        assert y["path"].any()  # the load yields: tangent solves ran
        assert not x["cols"].any()  # the sequential columns report no count of their own
        solved = y["path"].astype(bool)
        assert not y["cols"][~solved].any()
        # the CG count is Newton's iterations plus the six columns'
        assert (y["cols"][solved].sum(1) <= y["cg_its"][solved]).all()
        if n > 2:
            assert (y["cols"][solved] > 0).all()
        else:
            assert not y["cols"].any() and not y["cg_its"].any()  # no interior dof: CGs of no iteration
        for q in range(8):
            assert np.array_equal(y["C"][q], y["C"][q].T)


# ---------------------------------------------------------------- 2. columns that stop at different iterations
def test_columns_stop_at_different_iterations():
    """the per-column gate is exercised: in one of the cells a point's six columns do not all take the
    same number of iterations.  The cell was not chosen in advance: CellRef solves densely and reports no
    CG counts.  On the first run (MI355X) a point's six counts differed by up to 3 on sphere n = 9
    (71 .. 75), 4 on sphere n = 10 (82 .. 88) and 6 on layer n = 9 (58 .. 64); DESIGN §20, Results."""
    spread = {}
    for typ, n in CELLS:
        cols = np.concatenate([s["cols"][s["path"].astype(bool)] for s in cell_run(typ, n, 1)])
        spread[(typ, n)] = int((cols.max(1) - cols.min(1)).max()) if len(cols) else 0
    print("largest difference between a point's column counts:", spread)
    assert max(spread.values()) > 0


# ---------------------------------------------------------------- 3. independence
def embedded(u1):
    """TG's: the 2x2x2 grid's element as the second element of a 3x2x2 grid whose first element is solved too"""
    big = np.zeros((2, 2, 3, 3))
    big[:, :, 1:, :] = u1.reshape(2, 2, 2, 3)
    big[:, :, 0, :] = TN.field((2, 2, 2), 9, 4e-3).reshape(2, 2, 2, 3)[:, :, 0, :]
    return big.ravel()


@functools.lru_cache(maxsize=None)
def base_n10():
    return run_stages(0, 10, 0, stages=(1.0,))


@pytest.mark.parametrize("poll,blocks,big", [(1, 0, False), (7, 0, False), (16, 0, False), (16, 3, False),
                                             (16, 0, True), (7, 3, True)])
def test_bits_do_not_depend_on_poll_batch_slot_or_grid(poll, blocks, big):
    base = base_n10()
    assert base[0]["cg_its"].max() > 16 * 7  # CGs longer than the poll intervals
    if big:
        out = run_stages(0, 10, 1, u1=embedded(load()), grid=(3, 2, 2), stages=(1.0,), micro_grid_poll=poll,
                         micro_mem_blocks=blocks)
        assert out[0]["path"][:8].all()  # the first element is solved too
        same_bits(base, out, slice(8, None))
    else:
        out = run_stages(0, 10, 1, stages=(1.0,), micro_grid_poll=poll, micro_mem_blocks=blocks)
        same_bits(base, out)
    assert np.array_equal(base[0]["sig"], cell_run(0, 10, 1)[0]["sig"])


# ---------------------------------------------------------------- 4. the failure path
def test_an_unconverged_cell_fails_as_today():
    """micro_max_it 3 bounds every CG of the cell, the six unit-strain solves of C_hom first: the call
    fails there, with code 33 and the message of the sequential setting.  (No option makes a tangent
    column alone run out of iterations: a limit that stops a column stops C_hom's or Newton's CG before.)"""
    u1 = load()
    seen = {}
    for tangent in (0, 1):
        with TG.grid_ctx(TN.nl_argv(0, 5), micro_nl_tangent=tangent, micro_max_it=3) as m:
            m.set_u(u1)
            m.set_strains()
            with pytest.raises(M.MacrocError, match=r"failed \(33\): -mat_law micro: the micro cell's CG did not converge "
                                                    r"for load case 0 \(unit strain component xx\): 3 iterations") as e:
                m.homogenize()
            seen[tangent] = str(e.value)
            m.set_option("micro_max_it", 0)  # back at the default: the same context goes on
            m.homogenize()
            seen[tangent, "sig"], seen[tangent, "C"] = m.stress().reshape(-1, 6), m.gp_ctan()
            seen[tangent, "info"] = m.micro_nl_info()
    assert seen[0] == seen[1]
    with TG.grid_ctx(TN.nl_argv(0, 5), micro_nl_tangent=1) as m:
        _, sig, Cg, info = TN.evaluate(m, u1)
    for tangent in (0, 1):
        assert np.array_equal(seen[tangent, "sig"], sig) and np.array_equal(seen[tangent, "C"], Cg)
        for k in ("path", "newton_its", "cg_its", "rnorm"):
            assert np.array_equal(seen[tangent, "info"][k], info[k])
    assert info["path"].all()
    msgs = []
    for tangent in (0, 1):  # a cell that Newton gives up on never reaches its columns: code 35, the same words
        with TG.grid_ctx(TN.nl_argv(0, 5), micro_nl_tangent=tangent, micro_nl_max_it=1) as m:
            m.set_u(u1)
            m.set_strains()
            with pytest.raises(M.MacrocError, match=r"failed \(35\): .*\d+ of 8 micro cells did not converge; worst: Gauss "
                                                    r"point \d+ \(Newton gave up\): 1 Newton iterations") as e:
                m.homogenize()
            msgs.append(str(e.value))
            assert not m.micro_nl_tangent_its().any()
            m.set_option("micro_nl_max_it", 20)
            m.homogenize()
            assert np.array_equal(m.stress().reshape(-1, 6), sig) and np.array_equal(m.gp_ctan(), Cg)
    assert msgs[0] == msgs[1]


# ---------------------------------------------------------------- 5. below yield
def test_below_yield_is_the_linear_grid_solver_bit_for_bit():
    grid = (5, 4, 3)
    u = TN.field(grid, 11, 2e-5)
    with TG.grid_ctx(TN.nl_argv(1, 9, grid), micro_nl_tangent=1) as a:
        ba, va = TN.assemble(a, u)
        sa, info = a.stress(), a.micro_nl_info()
        assert not info["path"].any() and info["slots"] == 0 and info["slots_used"] == 0
        assert not a.micro_nl_tangent_its().any()
    with M.Macroc(TN.nl_argv(1, 9, grid, law="micro", extra=("-micro_solver", "grid"))) as b:
        bb, vb = TN.assemble(b, u)
        sb = b.stress()
    assert np.linalg.norm(bb) > 0
    assert np.array_equal(sa, sb) and np.array_equal(ba, bb) and np.array_equal(va, vb)


# ---------------------------------------------------------------- 6. with the globalised Newton
def test_start_and_line_search_with_block():
    """DESIGN §19's sphere cell (n = 12, one strain, e0 -> commit -> 1.25 e0) with micro_nl_start 1 and
    micro_nl_ls 5: a round may hold two transitions, the step's x is kept through its trials."""
    u1 = TN.field((2, 2, 2), 5, 4e-3, wobble=0)
    seq, blk = (run_stages(0, 12, t, u1=u1, stages=(1.0, 1.25), micro_nl_start=1, micro_nl_ls=5) for t in (0, 1))
    same_bits(seq, blk)
    for x, y in zip(seq, blk):
        assert np.array_equal(x["steps"]["ls_rejects"], y["steps"]["ls_rejects"])
        assert np.array_equal(x["steps"]["min_step"], y["steps"]["min_step"])
        assert y["path"].all() and (y["rnorm"] <= TN.NL_RTOL).all()


# ---------------------------------------------------------------- 7. solver 0 keeps its columns
@pytest.mark.parametrize("mem", [0, 1])
def test_solver_0_takes_the_option_without_effect(mem):
    u1, out = load(), []
    for tangent in (0, 1):
        with M.Macroc(TN.nl_argv(0, 4)) as m:
            m.set_option("micro_mem", mem)
            m.set_option("micro_nl_tangent", tangent)
            before = m.get_info()["device_bytes"]
            out.append(TN.evaluate(m, u1) + (m.micro_nl_tangent_its(), m.get_info()["device_bytes"] - before))
            assert m.micro_nl_tangent() == tangent
    for x, y in zip(*out):
        if isinstance(x, dict):
            assert all(np.array_equal(x[k], y[k]) for k in x)
        else:
            assert np.array_equal(x, y)
    assert out[1][3]["path"].all() and not out[1][4].any()


# ---------------------------------------------------------------- 8. memory
def test_workspace_is_counted_and_released():
    n, u1 = 10, TN.field((2, 2, 2), 5, 4e-6)  # below yield: no slot, the options stay free
    # 8 solves share a launch (the 8 Gauss points): five more columns' x, r, p, q, five more sets of work
    # stresses, six columns' eight partial-sum arrays (8 tiles) and six 56-byte column records each
    block = 8 * (8 * (5 * 4 * 3 * n ** 3 + 5 * 6 * 8 * (n - 1) ** 3 + 6 * 8 * 8) + 6 * 56)
    with M.Macroc(TN.nl_argv(0, n)) as m:
        before = m.get_info()["device_bytes"]
        m.set_option("micro_nl_tangent", 1)  # solver 0: nothing to lay out
        assert m.get_info()["device_bytes"] == before
        m.set_option("micro_nl_tangent", 0)
        m.set_option("micro_nl_solver", 1)
        _, _, _, info = TN.evaluate(m, u1)
        assert not info["path"].any() and info["slots"] == 0
        seq = m.get_info()["device_bytes"]
        fields = (6 * 3 * n ** 3 + 38 * 8 * (n - 1) ** 3) * 8  # the unit-strain fields and concentration tensors stay
        assert seq - before - fields >= 8 * 6 * 3 * n ** 3 * 8
        m.set_option("micro_nl_tangent", 1)
        assert m.get_info()["device_bytes"] == seq + block
        TN.evaluate(m, u1)
        assert m.get_info()["device_bytes"] == seq + block
        m.set_option("micro_nl_tangent", 0)
        assert m.get_info()["device_bytes"] == seq
        m.set_option("micro_nl_tangent", 1)
        m.set_option("micro_nl_solver", 0)
        assert m.get_info()["device_bytes"] == before + fields
        m.set_option("micro_nl_solver", 1)  # block still: laid out at the next solve
        TN.evaluate(m, u1)
        assert m.get_info()["device_bytes"] == seq + block


# ---------------------------------------------------------------- 9. the option's values, words and rule
def test_option_values_words_and_slots_in_use():
    u1 = load()
    with TG.grid_ctx(TN.nl_argv(0, 4)) as m:
        assert m.micro_nl_tangent() == 0
        for bad in (2, -1, 0.5):
            with pytest.raises(M.MacrocError, match=r"micro_nl_tangent: 0 \(seq.*\) or 1 \(block.*\)"):
                m.set_option("micro_nl_tangent", bad)
            assert M.lib().mcx_set_option(m._ctx, b"micro_nl_tangent", float(bad)) == 1
        assert m.micro_nl_tangent() == 0
        sig0 = TN.evaluate(m, u1)[1]
        with pytest.raises(M.MacrocError, match="micro_nl_tangent: 8 history slots are in use"):
            m.set_option("micro_nl_tangent", 1)
        assert M.lib().mcx_set_option(m._ctx, b"micro_nl_tangent", 1.0) == 2
        m.set_option("micro_nl_tangent", 0)  # no change: accepted
        assert m.micro_nl_tangent() == 0 and np.array_equal(TN.evaluate(m, u1)[1], sig0)
    with TG.grid_ctx(TN.nl_argv(0, 4), micro_nl_tangent=1) as m:
        assert np.array_equal(TN.evaluate(m, u1)[1], sig0)
        with pytest.raises(M.MacrocError, match="micro_nl_tangent: 8 history slots are in use"):
            m.set_option("micro_nl_tangent", 0)
        assert m.micro_nl_tangent() == 1 and np.array_equal(TN.evaluate(m, u1)[1], sig0)
    for where in (M.parse_args, M.Macroc):
        with pytest.raises(M.MacrocError, match="-micro_nl_tangent: seq or block, got grid"):
            where(TN.nl_argv(0, 4, extra=("-micro_nl_tangent", "grid")))
    for word, value in (("seq", 0), ("block", 1)):  # the flag is the option (mcx_apply_args)
        with M.Macroc(TN.nl_argv(0, 4, extra=("-micro_nl_solver", "grid", "-micro_nl_tangent", word))) as m:
            assert m.micro_nl_tangent() == value
            assert np.array_equal(TN.evaluate(m, u1)[1], sig0)
            assert m.micro_nl_tangent_its().any() == bool(value)
    for law in ("micro", "elastic"):  # accepted, no effect
        res = []
        for tangent in (0, 1):
            with M.Macroc(TN.nl_argv(0, 4, law=law)) as m:
                m.set_option("micro_nl_tangent", tangent)
                assert m.micro_nl_tangent() == tangent
                m.set_u(u1)
                m.set_strains()
                m.homogenize()
                res.append(m.stress())
        assert np.array_equal(*res)


# ---------------------------------------------------------------- 10. driver
def test_driver_takes_the_flag(tmp_path):
    """the README's -micro_nl_solver grid command at -micro_n 10: with -micro_nl_tangent block the time
    loop runs to its end and prints the lines of the seq run (all but the elapsed time)."""
    exe = os.path.join(ROOT, "macroc_amd", "driver", "macroc_amd")
    argv = [exe, "-da_grid_x", "4", "-da_grid_y", "4", "-da_grid_z", "4", "-ts", "2", "-mat_law", "micro_nl",
            "-micro_n", "10", "-micro_nl_solver", "grid", "-micro_type", "0", "-micro_mat_1", "1e7,0.25,7.6e3,1e8",
            "-micro_mat_2", "1e8,0.3,1e9,1e7"]
    logs = {}
    for word in ("seq", "block"):
        d = tmp_path / word
        d.mkdir()
        out = subprocess.run(argv + ["-micro_nl_tangent", word], cwd=d, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "options you set that were not used" not in out.stderr and "has no effect" not in out.stderr
        assert "Elapsed time" in out.stdout
        logs[word] = [l for l in out.stdout.splitlines() if not l.startswith("Elapsed time")]
    counts = [int(l.split(":")[1].split()[0]) for l in logs["block"] if l.startswith("Non-Linear Gauss points : ")]
    assert counts and max(counts) > 0, logs["block"]
    assert logs["seq"] == logs["block"]
