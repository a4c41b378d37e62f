"""Option micro_nl_apply 1 (-micro_nl_apply fused): a CG iteration of micro_nl_solver 1 forms
q = K_T p and the tiles' p.q in one launch (k_mnlg_apply, k_mnlb_apply under micro_nl_tangent 1) that
marches a tile's element layers with one layer of stresses in LDS and never writes the work stresses.
Every node's 64 terms are added in mnl_gather_sig's order, so the option changes no bit: every
comparison here is np.array_equal, never a tolerance.

The materials, the load and the helpers are test_gpu_micro_nl_grid's and test_gpu_micro_nl_block's
(load (5, 4e-3) through 1.0 -> commit -> 1.5 -> commit -> 0.5).  A run is made once per (cell, tangent,
apply) and shared.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import macroc_amd as M
import test_gpu_micro_nl as TN
import test_gpu_micro_nl_grid as TG
import test_gpu_micro_nl_block as TB

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# sphere n = 9: one full element tile and a second node tile of one node per axis; sphere n = 10: two partial
# tiles per axis; a layer; one interior node; no interior dof
CELLS = [(0, 9), (0, 10), (1, 9), (1, 3), (1, 2)]
KEYS = TB.KEYS


def run_stages(typ, n, tangent, apply, u1=None, grid=(2, 2, 2), stages=TN.STAGES, switch=None, **opts):
    """TB.run_stages with the option micro_nl_apply (switch: its value per stage, set before the stage)"""
    u1 = TB.load() if u1 is None else u1
    out = []
    with TG.grid_ctx(TN.nl_argv(typ, n, grid), micro_nl_tangent=tangent, micro_nl_apply=apply, **opts) as m:
        assert m.micro_nl_tangent() == tangent and m.micro_nl_apply() == apply
        for st, fac in enumerate(stages):
            if switch is not None:
                m.set_option("micro_nl_apply", switch[st])
                assert m.micro_nl_apply() == switch[st]
            eps, sig, Cg, info = TN.evaluate(m, fac * u1)
            out.append(dict(eps=eps, sig=sig, C=Cg, f=np.array(m.nonlinear_stats()[1]), path=info["path"],
                            newton_its=info["newton_its"], cg_its=info["cg_its"], rnorm=info["rnorm"],
                            cols=m.micro_nl_tangent_its(), steps=m.micro_nl_steps(), launches=m.micro_nl_apply_launches(),
                            apply=m.micro_nl_apply()))
            m.update_vars()
    return out


@functools.lru_cache(maxsize=None)
def cell_run(typ, n, tangent, apply, stages=TN.STAGES):
    return run_stages(typ, n, tangent, apply, stages=stages)


def same_bits(a, b, sel=None):
    """TB.same_bits and the steps of the globalised loop"""
    assert len(a) == len(b)
    TB.same_bits(a, b, sel)
    for x, y in zip(a, b):
        for k in ("ls_rejects", "min_step"):
            assert np.array_equal(x["steps"][k], y["steps"][k] if sel is None else y["steps"][k][sel]), k


def check_launches(runs, n):
    for r in runs:
        if r["apply"] and r["path"].any() and n > 2:
            assert r["launches"] > 0
        if not r["apply"]:
            assert r["launches"] == 0


# ---------------------------------------------------------------- 1. fused gives the split bits
@pytest.mark.parametrize("tangent", [0, 1])
@pytest.mark.parametrize("typ,n", CELLS)
def test_fused_gives_the_split_bits(typ, n, tangent):
    split, fused = cell_run(typ, n, tangent, 0), cell_run(typ, n, tangent, 1)
    assert len(split) == len(fused) == 3
    same_bits(split, fused)
    for st, (x, y) in enumerate(zip(split, fused)):
        print(f"cell ({typ},{n}) tangent {tangent} stage {st}: newton {y['newton_its']} cg {y['cg_its']} "
              f"fused launches {y['launches']}")
        assert y["path"].any()  # the load yields: CGs ran
        assert np.array_equal(x["cols"], y["cols"])
    check_launches(split, n)
    check_launches(fused, n)


@pytest.mark.parametrize("typ,n", CELLS)
def test_block_fused_gives_the_sequential_split_bits(typ, n):
    ref, both = cell_run(typ, n, 0, 0), cell_run(typ, n, 1, 1)
    same_bits(ref, both)
    for x, y in zip(both, cell_run(typ, n, 1, 0)):
        assert np.array_equal(x["cols"], y["cols"])  # micro_nl_tangent_its()
        if n > 2:
            assert (x["cols"][x["path"].astype(bool)] > 0).all()


@pytest.mark.parametrize("tangent", [0, 1])
def test_three_tiles_per_axis(tangent):
    """sphere n = 17: the smallest cell whose middle tile has neighbours on both sides and whose last tile
    holds boundary nodes only (it writes a partial of 0 without element work)"""
    split, fused = (cell_run(0, 17, tangent, f, stages=(1.0,)) for f in (0, 1))
    same_bits(split, fused)
    assert np.array_equal(split[0]["cols"], fused[0]["cols"])
    print("n = 17: newton", fused[0]["newton_its"], "cg", fused[0]["cg_its"], "fused launches", fused[0]["launches"])
    assert fused[0]["path"].all() and (fused[0]["rnorm"] <= TN.NL_RTOL).all()
    check_launches(split, 17)
    check_launches(fused, 17)
    if tangent:
        same_bits(cell_run(0, 17, 0, 0, stages=(1.0,)), fused)


# ---------------------------------------------------------------- 2. switching mid-history
def test_switching_with_slots_in_use():
    ref = cell_run(0, 10, 0, 0)
    out = run_stages(0, 10, 0, 0, switch=(0, 1, 0))
    same_bits(ref, out)
    assert [r["apply"] for r in out] == [0, 1, 0]
    assert out[0]["launches"] == 0 and out[1]["launches"] > 0 and out[2]["launches"] == 0


# ---------------------------------------------------------------- 3. independence
@pytest.mark.parametrize("poll,blocks,big", [(1, 0, False), (7, 0, False), (16, 0, False), (16, 3, False),
                                             (16, 0, True), (7, 3, True)])
def test_bits_do_not_depend_on_poll_batch_slot_or_grid(poll, blocks, big):
    base = TB.base_n10()  # split, sequential columns
    if big:
        out = run_stages(0, 10, 0, 1, u1=TB.embedded(TB.load()), grid=(3, 2, 2), stages=(1.0,), micro_grid_poll=poll,
                         micro_mem_blocks=blocks)
        assert out[0]["path"][:8].all()  # the first element is solved too
        same_bits(base, out, slice(8, None))
    else:
        out = run_stages(0, 10, 0, 1, stages=(1.0,), micro_grid_poll=poll, micro_mem_blocks=blocks)
        same_bits(base, out)
    assert out[0]["launches"] > 0


# ---------------------------------------------------------------- 4. with the globalised Newton
def test_start_and_line_search_with_fused():
    """DESIGN §19's sphere cell (n = 12, one strain, e0 -> commit -> 1.25 e0) with micro_nl_start 1 and
    micro_nl_ls 5"""
    u1 = TN.field((2, 2, 2), 5, 4e-3, wobble=0)
    split, fused = (run_stages(0, 12, 0, f, u1=u1, stages=(1.0, 1.25), micro_nl_start=1, micro_nl_ls=5) for f in (0, 1))
    same_bits(split, fused)
    for y in fused:
        assert y["path"].all() and (y["rnorm"] <= TN.NL_RTOL).all() and y["launches"] > 0


# ---------------------------------------------------------------- 5. the failure paths
def test_failures_are_todays():
    u1 = TB.load()
    seen = {}
    for apply in (0, 1):
        with TG.grid_ctx(TN.nl_argv(0, 5), micro_nl_apply=apply, micro_max_it=3) as m:
            m.set_u(u1)
            m.set_strains()
            with pytest.raises(M.MacrocError, match=r"failed \(33\): -mat_law micro: the micro cell's CG did not converge "
                                                    r"for load case 0 \(unit strain component xx\): 3 iterations") as e:
                m.homogenize()
            seen[apply] = str(e.value)
            m.set_option("micro_max_it", 0)  # back at the default: the same context goes on
            m.homogenize()
            seen[apply, "sig"], seen[apply, "C"] = m.stress().reshape(-1, 6), m.gp_ctan()
            seen[apply, "info"] = m.micro_nl_info()
    assert seen[0] == seen[1]
    with TG.grid_ctx(TN.nl_argv(0, 5)) as m:  # a fresh context, split
        _, sig, Cg, info = TN.evaluate(m, u1)
    for apply in (0, 1):
        assert np.array_equal(seen[apply, "sig"], sig) and np.array_equal(seen[apply, "C"], Cg)
        for k in ("path", "newton_its", "cg_its", "rnorm"):
            assert np.array_equal(seen[apply, "info"][k], info[k])
    assert info["path"].all()
    msgs = []
    for apply in (0, 1):
        with TG.grid_ctx(TN.nl_argv(0, 5), micro_nl_apply=apply, micro_nl_max_it=1) as m:
            m.set_u(u1)
            m.set_strains()
            with pytest.raises(M.MacrocError, match=r"failed \(35\): .*\d+ of 8 micro cells did not converge; worst: Gauss "
                                                    r"point \d+ \(Newton gave up\): 1 Newton iterations") as e:
                m.homogenize()
            msgs.append(str(e.value))
            m.set_option("micro_nl_max_it", 20)
            m.homogenize()
            assert np.array_equal(m.stress().reshape(-1, 6), sig) and np.array_equal(m.gp_ctan(), Cg)
            assert (m.micro_nl_apply_launches() > 0) == bool(apply)
    assert msgs[0] == msgs[1]


# ---------------------------------------------------------------- 6. the cases without effect
@pytest.mark.parametrize("mem", [0, 1])
def test_solver_0_takes_the_option_without_effect(mem):
    u1, out = TB.load(), []
    for apply in (0, 1):
        with M.Macroc(TN.nl_argv(0, 4)) as m:
            m.set_option("micro_mem", mem)
            m.set_option("micro_nl_apply", apply)
            out.append(TN.evaluate(m, u1))
            assert m.micro_nl_apply() == apply and m.micro_nl_apply_launches() == 0
    for x, y in zip(*out):
        if isinstance(x, dict):
            assert all(np.array_equal(x[k], y[k]) for k in x)
        else:
            assert np.array_equal(x, y)
    assert out[1][3]["path"].all()


def test_below_yield_is_the_linear_grid_solver_bit_for_bit():
    grid = (5, 4, 3)
    u = TN.field(grid, 11, 2e-5)
    with TG.grid_ctx(TN.nl_argv(1, 9, grid), micro_nl_apply=1) as a:
        ba, va = TN.assemble(a, u)
        sa, info = a.stress(), a.micro_nl_info()
        assert not info["path"].any() and info["slots"] == 0 and info["slots_used"] == 0
        assert a.micro_nl_apply_launches() == 0
    with M.Macroc(TN.nl_argv(1, 9, grid, law="micro", extra=("-micro_solver", "grid"))) as b:
        bb, vb = TN.assemble(b, u)
        sb = b.stress()
    assert np.linalg.norm(bb) > 0
    assert np.array_equal(sa, sb) and np.array_equal(ba, bb) and np.array_equal(va, vb)


@pytest.mark.parametrize("tangent", [0, 1])
def test_device_bytes_and_values(tangent):
    u1 = TB.load()
    with TG.grid_ctx(TN.nl_argv(0, 4), micro_nl_tangent=tangent) as m:
        assert m.micro_nl_apply() == 0
        sig0 = TN.evaluate(m, u1)[1]  # the workspace exists, slots are in use
        dev = m.get_info()["device_bytes"]
        for bad in (2, -1, 0.5):
            with pytest.raises(M.MacrocError, match=r"micro_nl_apply: 0 \(split.*\) or 1 \(fused.*\)"):
                m.set_option("micro_nl_apply", bad)
            assert M.lib().mcx_set_option(m._ctx, b"micro_nl_apply", float(bad)) == 1
        assert m.micro_nl_apply() == 0
        m.set_option("micro_nl_apply", 1)
        assert m.micro_nl_apply() == 1 and m.get_info()["device_bytes"] == dev
        assert np.array_equal(TN.evaluate(m, u1)[1], sig0) and m.micro_nl_apply_launches() > 0
        assert m.get_info()["device_bytes"] == dev
        m.set_option("micro_nl_apply", 0)
        assert m.get_info()["device_bytes"] == dev
        assert np.array_equal(TN.evaluate(m, u1)[1], sig0) and m.micro_nl_apply_launches() == 0
    for where in (M.parse_args, M.Macroc):
        with pytest.raises(M.MacrocError, match="-micro_nl_apply: split or fused, got grid"):
            where(TN.nl_argv(0, 4, extra=("-micro_nl_apply", "grid")))
    for word, value in (("split", 0), ("fused", 1)):  # the flag is the option (mcx_apply_args)
        with M.Macroc(TN.nl_argv(0, 4, extra=("-micro_nl_solver", "grid", "-micro_nl_apply", word))) as m:
            assert m.micro_nl_apply() == value
            assert np.array_equal(TN.evaluate(m, u1)[1], sig0)
            assert (m.micro_nl_apply_launches() > 0) == bool(value)


# ---------------------------------------------------------------- 7. the driver
def test_driver_takes_the_flag(tmp_path):
    """the README's -micro_nl_solver grid command at -micro_n 10: with -micro_nl_apply fused the time loop
    prints the lines of the split run (all but the elapsed time)."""
    exe = os.path.join(ROOT, "macroc_amd", "driver", "macroc_amd")
    argv = [exe, "-da_grid_x", "4", "-da_grid_y", "4", "-da_grid_z", "4", "-ts", "2", "-mat_law", "micro_nl",
            "-micro_n", "10", "-micro_nl_solver", "grid", "-micro_type", "0", "-micro_mat_1", "1e7,0.25,7.6e3,1e8",
            "-micro_mat_2", "1e8,0.3,1e9,1e7"]
    logs = {}
    for word in ("split", "fused"):
        d = tmp_path / word
        d.mkdir()
        out = subprocess.run(argv + ["-micro_nl_apply", word], cwd=d, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "options you set that were not used" not in out.stderr and "has no effect" not in out.stderr
        assert "Elapsed time" in out.stdout
        logs[word] = [l for l in out.stdout.splitlines() if not l.startswith("Elapsed time")]
    counts = [int(l.split(":")[1].split()[0]) for l in logs["fused"] if l.startswith("Non-Linear Gauss points : ")]
    assert counts and max(counts) > 0, logs["fused"]
    assert logs["split"] == logs["fused"]
