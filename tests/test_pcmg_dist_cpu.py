"""The distributed multigrid hierarchy (option pc_mg_dist) without a GPU: mcx_pc_mg_plan against a
Python restatement of the ownership rule and of PETSc's DMDA split, the automatic early stop, the
refusal of a fixed level count that reaches a rank without nodes, the flag, the ABI, and the planner
(macroc_amd/csrc/pcmg_plan.h) in a stand-alone program under AddressSanitizer + UBSan.

The rule (include/macroc_amd.h): coarse node I of an axis of N > 2 nodes sits on fine node
min(2 I, N - 1) and belongs to the owner of that fine node; the fine ranges are the DMDA's."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import macroc_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the rule, restated
def axis_coarse(N):
    """fine indices of the coarse nodes of an axis"""
    if N <= 2:
        return list(range(N))
    c = list(range(0, N, 2))
    if (N - 1) % 2:
        c.append(N - 1)
    return c


def dmda_split(N, P):
    out, s = [], 0
    for r in range(P):
        n = N // P + (1 if N % P > r else 0)
        out.append((s, s + n))
        s += n
    return out


def axis_levels(N, P, nlev):
    """[(N_l, [(start, end) per rank column])] for nlev levels of an axis"""
    rng, out = dmda_split(N, P), []
    for _ in range(nlev):
        out.append((N, rng))
        c = axis_coarse(N)
        rng = [([I for I, f in enumerate(c) if s <= f < e] or [0, -1]) for s, e in rng]
        rng = [(idx[0], idx[-1] + 1) for idx in rng]
        N = len(c)
    return out


def argv_of(grid, ranks):
    return ["-da_grid_x", grid[0], "-da_grid_y", grid[1], "-da_grid_z", grid[2], "-da_processors_x", ranks[0],
            "-da_processors_y", ranks[1], "-da_processors_z", ranks[2]]


CASES = [((17, 9, 9), (2, 1, 1)), ((16, 9, 9), (2, 1, 1)), ((24, 9, 9), (3, 1, 1)), ((33, 9, 9), (4, 1, 1)),
         ((13, 9, 9), (2, 1, 1)), ((20, 9, 9), (3, 1, 1)), ((16, 16, 16), (2, 2, 2))]


@pytest.mark.parametrize("grid,ranks", CASES, ids=lambda v: "x".join(map(str, v)))
def test_plan_against_the_rule(grid, ranks):
    nr = int(np.prod(ranks))
    plans = [M.pc_mg_plan(argv_of(grid, ranks), rank=r) for r in range(nr)]
    nlev = len(plans[0][0])
    assert nlev >= 2 and all(len(s) == nlev == len(n) for s, n in plans)
    want = [axis_levels(grid[a], ranks[a], nlev) for a in range(3)]
    for r, (start, count) in enumerate(plans):
        col = (r % ranks[0], (r // ranks[0]) % ranks[1], r // (ranks[0] * ranks[1]))
        for l, a in itertools.product(range(nlev), range(3)):
            s, e = want[a][l][1][col[a]]
            assert (start[l][a], start[l][a] + count[l][a]) == (s, e), (r, l, a)
    for l in range(nlev):
        N = [want[a][l][0] for a in range(3)]
        # the boxes tile the level exactly: every node in exactly one box
        seen = np.zeros(N[::-1], dtype=int)
        for start, count in plans:
            s, n = start[l], count[l]
            assert np.all(n >= 1)
            seen[s[2]:s[2] + n[2], s[1]:s[1] + n[1], s[0]:s[0] + n[0]] += 1
        assert np.all(seen == 1), (l, N)
        if l + 1 == nlev:
            continue
        # one ghost layer suffices, per axis: P's coarse parents of an owned fine node and P^T's fine
        # children of an owned coarse node lie in the owned range or one node beside it
        for a in range(3):
            if N[a] <= 2:
                continue
            c = axis_coarse(N[a])
            pos = {f: q for q, f in enumerate(c)}
            for q in range(ranks[a]):
                (s, e), (cs, ce) = want[a][l][1][q], want[a][l + 1][1][q]
                for f in range(N[a]):
                    need = [pos[f]] if f in pos else [pos[f - 1], pos[f + 1]]
                    if s <= f < e:
                        assert all(cs - 1 <= I <= ce for I in need), (l, a, q, f)
                    for I in need:
                        if cs <= I < ce:
                            assert s - 1 <= f <= e, (l, a, q, I, f)


def test_automatic_levels_stop_before_an_empty_rank():
    grid = (24, 9, 40)
    for r in range(3):
        start, count = M.pc_mg_plan(argv_of(grid, (3, 1, 1)), rank=r)
        assert len(start) == 4
        assert count[:, 0].tolist() == [[8, 4, 2, 1], [8, 4, 2, 1], [8, 5, 3, 2]][r]
        assert count[:, 1:].tolist() == [[9, 40], [5, 21], [3, 11], [2, 6]]  # the levels (24,9,40) ... (4,2,6)
    start, count = M.pc_mg_plan(argv_of(grid, (1, 1, 1)))
    assert count.tolist() == [[24, 9, 40], [13, 5, 21], [7, 3, 11], [4, 2, 6], [3, 2, 4]] and not start.any()


def test_fixed_levels_reaching_an_empty_rank_refuse():
    argv = argv_of((12, 9, 9), (4, 1, 1))
    msgs = set()
    for r in range(4):
        with pytest.raises(M.MacrocError, match=r"failed \(2\).*level 3.*rank 1 without a node on axis x") as e:
            M.pc_mg_plan(argv, rank=r, levels=4)
        msgs.add(str(e.value))
    assert len(msgs) == 1  # every rank refuses alike
    assert len(M.pc_mg_plan(argv, rank=1, levels=3)[0]) == 3
    assert len(M.pc_mg_plan(argv, rank=1)[0]) == 3  # automatic: the same stop
    # a coarsest level above 3072 dofs is refused as on one rank
    with pytest.raises(M.MacrocError, match=r"failed \(2\).*14739 dofs.*3072.* 3 levels fit"):
        M.pc_mg_plan(argv_of((33, 33, 33), (2, 1, 1)), levels=2)
    # bad arguments: code 1
    for argv, kw in ((argv_of((9, 9, 9), (0, 1, 1)), {}), (argv_of((9, 9, 9), (2, 1, 1)), {"rank": 2}),
                     (argv_of((9, 9, 9), (2, 1, 1)), {"levels": 1}), (argv_of((9, 9, 9), (2, 1, 1)), {"levels": 17})):
        with pytest.raises(M.MacrocError, match=r"failed \(1\)"):
            M.pc_mg_plan(argv, **kw)


def test_parse_args_takes_the_flag(capfd):
    o = M.parse_args(["-da_grid_x", "17", "-pc_mg_dist", "1", "-pc_type", "mg", "-ksp_rtol", "1e-8"])
    assert o.NX == 17 and o.ksp_rtol == 1e-8  # the flags around it are still read
    assert "not used" not in capfd.readouterr().err


def test_abi_revision_and_opts_layout_unchanged():
    assert M.lib().mcx_abi_version() == 3 == M.ABI_VERSION
    assert C.sizeof(M.Opts) == 264


def test_new_entries_refuse_a_null_context():
    L = M.lib()
    assert L.mcx_pc_mg_box(None, 0, None, None) == 1
    assert L.mcx_pc_mg_plan(None, 0, 0, None, None, None) == 1
    assert L.mcx_set_option(None, b"pc_mg_dist", 1.0) != 0


def test_planner_under_sanitizers(tmp_path):
    """the stand-alone program tests/csrc/pcmg_plan_check.cpp, built by the Makefile's pcmg-plan-check
    with -fsanitize=address,undefined: the planner over the cases above and more, no report"""
    assert shutil.which("make") and (shutil.which("g++") or shutil.which("clang++")), "no host tool chain"
    exe = str(tmp_path / "pcmg_plan_check")
    more = [] if shutil.which("g++") else ["HOSTCXX=clang++"]
    subprocess.run(["make", "-s", "-C", ROOT, "pcmg-plan-check", "PCMG_PLAN_CHECK=" + exe, *more], check=True,
                   capture_output=True, text=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("0 failures"), out.stdout + out.stderr
    out = subprocess.run([exe, "12", "9", "9", "4", "1", "1", "4"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "axis x" in out.stdout and "0 failures" in out.stdout, out.stdout + out.stderr
    out = subprocess.run([exe, "16", "16", "16", "2", "2", "2"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "3 levels" in out.stdout, out.stdout + out.stderr
