"""The matrix's life across re-assemblies as the exception-node set moves, grows and overflows.

One context per test lives through a sequence of hand-placed states (tests/reassembly_cases.py; their
preconditions are proven on the oracle by tests/test_reassembly_cases_cpu.py).  After every
assembly_jac the context is held against

  the oracle, bit for bit: b, the matrix dump, the SpMV under vi_fma 0 (value-indexed or AIJ blocks;
  the AIJ-split storage and the fused multiply-add rows within 1e-14 sum |a||x| per row, the bars of
  test_aij_split_single_rank / test_aij_vi_exception_nodes);
  itself under the settings that must give the same rows (vi_st 1 / 0 / -1, vi_st_dma, the exception
  kernel's forms, vi_st_l16, the structures built lazily after an assembly under vi_st 0, cg_dix);
  a FRESH context of the same argv and options assembled once at this state, bit for bit: dump, both
  SpMVs, the solve (its, rnorm, du) and the info fields.  device_bytes is left out (grown buffers
  stay); the documented latches (vi_declined, split_declined) are the only other difference allowed,
  and only the steps marked "latched" expect one.

Once per sequence, at its last state, the solve is also held against the oracle's.

The sequences run on (70, 20, 12) with the default staging rule (which gathers x on so flat a grid)
and with vi_stage 1 (64 x 16 tiles: the default-stencil march), and on (130, 9, 12) with vi_stage 1 and
vi_tx 0 / 128.
"""
from collections import namedtuple

import numpy as np
import pytest

import macroc_amd as M
import reassembly_cases as R

pytestmark = pytest.mark.gpu

Cfg = namedtuple("Cfg", "id grid options tile")
CONFIGS = [
    Cfg("g70", "g70", (), None),
    Cfg("g70-staged", "g70", (("vi_stage", 1),), (64, 16)),
    Cfg("g130-tx0", "g130", (("vi_stage", 1), ("vi_tx", 0)), (64, 16)),
    Cfg("g130-tx128", "g130", (("vi_stage", 1), ("vi_tx", 128)), (128, 8)),
]
INFO_FIELDS = ("storage", "vi_values", "vi_bits", "vi_blocks", "vi_exc_nodes", "st_listed", "spmv_tx", "spmv_ty",
               "spmv_kc")


def assemble(m, u):
    m.set_u(u)
    m.set_strains()
    m.homogenize()
    m.assembly_res()
    m.assembly_jac()


def set_options(m, cfg, seq):
    for k, v in cfg.options + tuple(seq.options):
        m.set_option(k, v)
    if seq.exc_max != R.VI_EXC_MAX:
        m.set_option("vi_exc_max", seq.exc_max)


def info_of(m):
    info = m.get_info()
    return {k: info[k] for k in INFO_FIELDS}


def snapshot(m, x):
    """What a context gives at its current matrix under the sequence's settings."""
    s = dict(b=m.b(), v=m.dump_csr()[2], info=info_of(m))
    m.set_option("vi_fma", 0)
    s["y0"] = m.spmv(x)
    m.set_option("vi_fma", 1)
    s["y1"] = m.spmv(x)
    s["its"], s["rnorm"], s["reason"] = m.solve_Ax()
    s["du"] = m.du()
    return s


def same_bits(a, b, what):
    for k in ("b", "v", "y0", "y1", "du"):
        assert np.array_equal(a[k], b[k]), (what, k)
    assert (a["its"], a["reason"]) == (b["its"], b["reason"]), what
    assert a["rnorm"] == b["rnorm"] or (np.isnan(a["rnorm"]) and np.isnan(b["rnorm"])), what
    assert a["info"] == b["info"], (what, a["info"], b["info"])


def against_oracle(s, ref, sel=slice(None)):
    """sel: the rank's owned dofs in the oracle's order"""
    assert np.array_equal(s["b"], ref.b[sel])
    storage = s["info"]["storage"]
    if storage == 2:  # AIJ-split: the rows within rounding
        assert np.all(np.abs(s["y0"] - ref.y[sel]) <= 1e-14 * ref.absrow[sel] + 1e-300)
    else:
        assert np.array_equal(s["y0"], ref.y[sel])
    assert np.all(np.abs(s["y1"] - ref.y[sel]) <= 1e-14 * ref.absrow[sel] + 1e-300)


def path_on(cfg, storage, state, nexc, nown, vi_st):
    """The SpMV takes the default-stencil path (get_info: st_listed >= 0): 64 x 16 staged tiles, the
    value-indexed storage, an interior representative left, and vi_st 1 or st_auto's rule."""
    if cfg.tile != (64, 16) or storage != 3 or R.CLASS_LOST.get(state) == 0:
        return False
    return vi_st == 1 or (vi_st < 0 and R.st_auto(nexc, nown))


def same_rows_under_settings(m, cfg, state, ref, s, nown):
    """The value-indexed matrix under every setting that must give the same rows; each restored."""
    x, y, y0, nexc = ref.x, s["y1"], s["y0"], ref.nexc

    def listed(vi_st):
        n = m.get_info()["st_listed"]
        on = path_on(cfg, 3, state, nexc, nown, vi_st)
        assert (n >= 0) == on, (state, vi_st, n)
        if on:  # the exception nodes among them; the whole list as the host restatement counts it
            assert n >= nexc and n == int(R.listed_model(cfg.grid, state).sum()), (state, vi_st, n)
        return n

    for st in (1, 0, -1):
        m.set_option("vi_st", st)
        assert np.array_equal(m.spmv(x), y), ("vi_st", st)
        listed(st)
    m.set_option("vi_st", 1)
    for dma in (0, 1, -1):
        m.set_option("vi_st_dma", dma)
        assert np.array_equal(m.spmv(x), y), ("vi_st_dma", dma)
    for l16 in (0, 1, -1):
        m.set_option("vi_st_l16", l16)
        assert np.array_equal(m.spmv(x), y), ("vi_st_l16", l16)
    m.set_option("vi_st", 0)
    for xk, xl in ((0, 0), (1, 2048)):
        m.set_option("vi_exc_kernel", xk)
        m.set_option("vi_exc_list", xl)
        assert np.array_equal(m.spmv(x), y), ("vi_exc", xk, xl)
        m.set_option("vi_fma", 0)
        assert np.array_equal(m.spmv(x), y0), ("vi_exc", xk, xl, "vi_fma 0")
        m.set_option("vi_fma", 1)
    # an assembly under vi_st 0 leaves the structures pending; vi_st 1 then builds them from this matrix
    m.assembly_jac()
    assert m.get_info()["st_listed"] == -1 and np.array_equal(m.spmv(x), y)
    m.set_option("vi_st", 1)
    assert np.array_equal(m.spmv(x), y), "st_pending"
    n1 = listed(1)
    m.set_option("vi_st", -1)
    assert np.array_equal(m.spmv(x), y)
    assert info_of(m) == s["info"], (info_of(m), s["info"])
    # the Jacobi diagonal index after the set moved: the same iteration count and du bits as the Jacobi vector
    m.set_option("cg_dix", 0)
    its, _, _ = m.solve_Ax()
    assert its == s["its"] and np.array_equal(m.du(), s["du"]), "cg_dix 0"
    m.set_option("cg_dix", 1)
    return n1


def run_sequence(cfg, seq, extra=None):
    """The long-lived context through seq; extra(q, step, m, snap, fresh, forced): a sequence's own checks
    (forced: st_listed under vi_st 1, None where the matrix is not value-indexed)."""
    grid = cfg.grid
    nown = int(np.prod(R.GRIDS[grid]))
    snaps = []
    refs = R.references(grid, [step.state for step in seq.steps])
    with M.Macroc(R.argv(grid)) as m:
        set_options(m, cfg, seq)
        exc_max, fell_to = seq.exc_max, None
        for q, step in enumerate(seq.steps):
            ref = refs[step.state]
            if step.option:
                name, value = step.option
                m.set_option(name, exc_max if value is None else value)
            assemble(m, ref.u)
            s = snapshot(m, ref.x)
            snaps.append(s)
            print(f"{cfg.id} step {q} {step.state}: {s['info']} its {s['its']} reason {s['reason']}")
            if cfg.tile and s["info"]["storage"] == 3:  # (the AIJ-split storage reports its own tile)
                assert (s["info"]["spmv_tx"], s["info"]["spmv_ty"]) == cfg.tile
            # the oracle
            assert np.array_equal(s["v"], ref.v)
            against_oracle(s, ref)
            # the info fields
            if step.storage == "vi":
                assert s["info"]["storage"] == 3 and s["info"]["vi_exc_nodes"] == ref.nexc, s["info"]
                on = path_on(cfg, 3, step.state, ref.nexc, nown, dict(seq.options).get("vi_st", -1))
                assert (s["info"]["st_listed"] >= 0) == on, s["info"]
                if on:
                    assert s["info"]["st_listed"] >= ref.nexc
            else:  # this assembly overflowed, or an earlier one did (the vi_declined latch)
                assert s["info"]["storage"] in (2, 0) and s["info"]["vi_exc_nodes"] == 0, s["info"]
                assert s["info"]["st_listed"] == -1
                if step.storage == "fallback":
                    fell_to = s["info"]["storage"]
                # a latched step keeps the storage the overflow took (blocks stay blocks: split_declined),
                # unless the step fixes another (an option cleared split_declined)
                want = step.code if step.code is not None else fell_to
                assert s["info"]["storage"] == want, (s["info"], want)
            # a fresh context at this state
            with M.Macroc(R.argv(grid)) as f:
                set_options(f, cfg, seq)
                assemble(f, ref.u)
                fs = snapshot(f, ref.x)
            if step.storage == "latched":  # the one allowed difference: the fresh context indexes this matrix
                assert fs["info"]["storage"] == 3 and fs["info"]["vi_exc_nodes"] == ref.nexc, fs["info"]
                assert np.array_equal(s["v"], fs["v"]) and np.array_equal(s["b"], fs["b"])
                assert s["reason"] == fs["reason"] and abs(s["its"] - fs["its"]) <= 1
                assert np.linalg.norm(s["du"] - fs["du"]) <= 50 * R.RTOL * np.linalg.norm(fs["du"])
            else:
                same_bits(s, fs, f"fresh context, step {q} {step.state}")
            if step.same_as is not None and seq.steps[step.same_as].storage == step.storage:
                same_bits(s, snaps[step.same_as], f"step {q} repeats step {step.same_as}")
            forced = None
            if s["info"]["storage"] == 3:
                forced = same_rows_under_settings(m, cfg, step.state, ref, s, nown)
            if extra:
                extra(q, step, m, s, fs, forced)
        # the solve against the oracle's, at the last state
        its, reason, du = ref.its, ref.reason, ref.du
        s = snaps[-1]
        assert s["reason"] > 0 and reason > 0 and abs(s["its"] - its) <= 1, (s["its"], its)
        assert np.linalg.norm(s["du"] - du) <= 50 * R.RTOL * np.linalg.norm(du)
    return snaps


cfgs = pytest.mark.parametrize("cfg", CONFIGS, ids=[c.id for c in CONFIGS])


@cfgs
def test_appear_move_vanish(cfg):
    """none -> one -> one moved -> none -> one: storage 3 with 0 exception nodes at none, nothing of the
    old site carried over, the last state the second bit for bit."""
    snaps = run_sequence(cfg, R.SEQUENCES["appear_move_vanish"])
    assert [s["info"]["vi_exc_nodes"] for s in snaps] == [0, 27, 27, 0, 27]
    assert all(s["info"]["storage"] == 3 for s in snaps)


@cfgs
def test_regrow_shrink(cfg):
    """one -> plane_J5 -> one -> plane_J5: the first step outgrows the capacity `one` left (the AoSoA
    layout of the exception blocks changes); after the shrink the same state runs under the larger one."""
    run_sequence(cfg, R.SEQUENCES["regrow_shrink"])


@cfgs
def test_cross_10_percent(cfg):
    """plane_J5 -> plane_half -> plane_J5 under vi_st -1: the default-stencil path on, off, on."""
    snaps = run_sequence(cfg, R.SEQUENCES["cross_10_percent"])
    if cfg.tile == (64, 16):
        assert [s["info"]["st_listed"] >= 0 for s in snaps] == [True, False, True]


@cfgs
@pytest.mark.parametrize("big", ["slab3", "all"])
def test_overflow_and_latch(cfg, big):
    """one -> slab3 (or all) -> one -> vi_exc_max set to its own value -> one: over vi_exc_max the
    matrix falls back (storage 2, or 0 where the split is refused) and stays exact; at the next `one` it
    is still not value-indexed (the vi_declined latch) and still exact; once the option is set it is
    value-indexed again and equals the fresh context."""
    snaps = run_sequence(cfg, R.SEQUENCES["overflow_and_latch_" + big])
    assert [s["info"]["storage"] == 3 for s in snaps] == [True, False, False, True]


@cfgs
def test_split_refused_and_cleared(cfg):
    """one -> slab3 -> one -> split_dense set -> one -> vi_exc_max set -> one, under split_dense 0: the
    overflow falls to AIJ blocks (storage 0) and stays there at `one` (vi_declined and split_declined);
    setting split_dense clears split_declined alone (AIJ-split, storage 2, exact); setting vi_exc_max
    clears vi_declined (storage 3, the first state's bits).  On these grids every matrix's corrections
    are dense, so under split_dense 0 none would fit the split again: the latch and a fresh refusal
    give the same storage, and what is pinned is that blocks stay blocks until the option is set."""
    snaps = run_sequence(cfg, R.SEQUENCES["split_refused_and_cleared"])
    assert [s["info"]["storage"] for s in snaps] == [3, 0, 0, 2, 3]


@cfgs
def test_representatives(cfg):
    """one -> the interior's middle candidate -> all five -> one: with the middle covered the path stays
    on and the middle node is listed; with all five covered the SpMV leaves the default-stencil path even
    under vi_st 1, the rows exact; back at `one` it is on again."""
    forced = []
    run_sequence(cfg, R.SEQUENCES["representatives"], lambda q, step, m, s, fs, n1: forced.append(n1))
    if cfg.tile == (64, 16):
        # (st_listed >= the exception nodes, the middle node among them, is asserted at every step)
        assert forced[0] >= 0 and forced[1] >= 0 and forced[2] == -1 and forced[3] == forced[0], forced


@cfgs
@pytest.mark.parametrize("face", ["zlo", "xhi"])
def test_face_class_lost(cfg, face):
    """one -> the five candidates of a face class -> one: the class unusable, every node of that face
    joins the listed rows (st_n jumps: st_l16's length rule, partials_fit and k_spmv_face's patch prefix
    sums see another size); it returns at `one`."""
    cls = {"zlo": 5, "xhi": 2}[face]
    forced, dirichlet = [], []

    def extra(q, step, m, s, fs, n1):
        forced.append(n1)
        if q == 0:
            dirichlet.append(np.unique(m.dump_dirichlet() // 3))

    seq = R.SEQUENCES["face_class_lost_" + face]
    run_sequence(cfg, seq, extra)
    if cfg.tile != (64, 16):
        return
    grid = cfg.grid
    on, nf, near = R.domain_masks(grid)
    inner = on[cls - 1] & (nf == 1)
    d = np.zeros(inner.size, dtype=bool)
    d[dirichlet[0]] = True
    assert np.array_equal(d, np.isin(np.arange(inner.size), np.unique(R.problem(grid).dirichlet_set() // 3)))
    NX, NY, NZ = R.GRIDS[grid]
    n_face = int(inner.sum())
    assert n_face == {5: (NX - 2) * (NY - 2), 2: (NY - 2) * (NZ - 2)}[cls]
    # the face's nodes listed anyway (Dirichlet rows or columns zeroed in their blocks: the Dirichlet nodes
    # and their neighbours); `one`'s exception nodes that leave the list
    before = R.listed_model(grid, "one")
    n_other = int((inner & before).sum())
    n_leave = int((R.closed_form_exc(grid, "one") & ~R.listed_model(grid, seq.steps[1].state)).sum())
    print(f"{cfg.id} {face}: st_listed {forced}, face nodes {n_face}, of them listed anyway {n_other}, leaving {n_leave}")
    assert n_other <= n_face // 5
    assert forced[1] - forced[0] >= n_face - n_other - n_leave, forced
    assert forced[1] >= n_face + int((nf > 1).sum())  # the face's nodes and the edge / corner nodes: all listed
    assert forced[2] == forced[0]


@cfgs
def test_lost_classes_first(cfg):
    """all five interior candidates -> the z-lo face's five -> one: the context's first build of the
    default-stencil structures has no usable class at all (zero coefficients), the second lacks the z-lo
    class, the third has all seven; the rows of a class that comes back are its representative's."""
    forced = []
    run_sequence(cfg, R.SEQUENCES["lost_first"], lambda q, step, m, s, fs, n1: forced.append(n1))
    if cfg.tile == (64, 16):
        assert forced[0] == -1 and forced[1] > forced[2] > 0, forced


@cfgs
def test_corners(cfg):
    """none -> bumps at (0, 0, 0) and (NX-1, NY-1, NZ-1) -> none: eight exception nodes each, all edge or
    corner nodes, on the last tile and the last plane."""
    snaps = run_sequence(cfg, R.SEQUENCES["corners"])
    assert [s["info"]["vi_exc_nodes"] for s in snaps] == [0, 16, 0]


# ---------------------------------------------------------------- two ranks
def two_rank_run(seq, fresh_of=None):
    """(130, 9, 12) over (2, 1, 1), in-process transport: per rank and step a snapshot; fresh_of: the one
    step a fresh group is assembled at."""
    from test_gpu_multirank import run_group

    grid = "g130"
    argv = R.argv(grid, "-da_processors_x", 2, "-da_processors_y", 1, "-da_processors_z", 1)
    steps = seq.steps if fresh_of is None else [seq.steps[fresh_of]]
    refs = R.references(grid, [step.state for step in steps])  # before the ranks' threads start

    def fn(m):
        m.set_option("vi_stage", 1)
        if seq.exc_max != R.VI_EXC_MAX:
            m.set_option("vi_exc_max", seq.exc_max)
        _, nat = m.owned_dofs()
        out = []
        for step in steps:
            ref = refs[step.state]
            assemble(m, ref.u[nat])
            rp = m.dump_csr(values=False)[0]
            s = snapshot(m, ref.x[nat])
            s.update(nat=nat, rp=rp)
            out.append(s)
        return out

    return run_group(argv, 2, fn)


def rows_equal(s, ref, grid):
    """a rank's rows against the oracle's in natural order (the columns are numbered per decomposition)"""
    rp1, _ = R.pattern(grid)
    for q, row in enumerate(s["nat"]):
        a, b = s["v"][s["rp"][q]:s["rp"][q + 1]], ref.v[rp1[row]:rp1[row + 1]]
        if not np.array_equal(np.sort(a.view(np.int64)), np.sort(b.view(np.int64))):
            return False
    return True


def check_two_ranks(name):
    grid = "g130"
    seq = R.SEQUENCES_2R[name]
    refs = R.references(grid, [step.state for step in seq.steps])
    long = two_rank_run(seq)
    for q, step in enumerate(seq.steps):
        ref = refs[step.state]
        fresh = two_rank_run(seq, fresh_of=q)
        latched_any = step.storage == "latched"
        du = np.zeros(len(ref.u))
        for r in (0, 1):
            s, fs = long[r][q], fresh[r][0]
            nexc = R.TWO_RANK_COUNTS[step.state][r]
            nown = len(s["nat"]) // 3
            over = R.overflows(nexc, nown, seq.exc_max)
            print(f"{name} step {q} {step.state} rank {r}: {s['info']} its {s['its']}")
            assert rows_equal(s, ref, grid)
            against_oracle(s, ref, s["nat"])
            du[s["nat"]] = s["du"]
            if over or (latched_any and r == 0):  # rank 0: over the limit, then latched
                assert s["info"]["storage"] in (2, 0) and s["info"]["vi_exc_nodes"] == 0, s["info"]
            else:
                assert s["info"]["storage"] == 3 and s["info"]["vi_exc_nodes"] == nexc, s["info"]
            if latched_any:  # the fresh group indexes both ranks' rows; rank 1's matrix and products the same bits
                assert fs["info"]["storage"] == 3 and fs["info"]["vi_exc_nodes"] == nexc
                assert np.array_equal(s["v"], fs["v"]) and np.array_equal(s["b"], fs["b"])
                if r == 1:
                    assert np.array_equal(s["y0"], fs["y0"]) and np.array_equal(s["y1"], fs["y1"])
                    assert s["info"] == fs["info"]
                assert abs(s["its"] - fs["its"]) <= 1
            else:
                same_bits(s, fs, f"{name}: fresh group, step {q}, rank {r}")
        # the solve of the mixed storages against the one-rank oracle
        its, reason, du1 = ref.its, ref.reason, ref.du
        assert long[0][q]["reason"] > 0 and reason > 0 and abs(long[0][q]["its"] - its) <= 1
        assert long[0][q]["its"] == long[1][q]["its"]
        assert np.linalg.norm(du - du1) <= 50 * R.RTOL * np.linalg.norm(du1)
    return long


def test_two_ranks_straddle_then_one_side():
    """A cube across the rank boundary, then on rank 1 alone (rank 0 goes from > 0 to 0 exception nodes:
    the exception array no longer passed), then on rank 0 alone."""
    long = check_two_ranks("straddle_then_one_side")
    assert [[s["info"]["vi_exc_nodes"] for s in long[r]] for r in (0, 1)] == [[9, 0, 27], [18, 27, 0]]


def test_two_ranks_one_rank_overflows():
    """one -> a slab on rank 0 over the lowered vi_exc_max (rank 1: one cube) -> one: the decision is
    per rank, so rank 0 holds its rows AIJ-split (or as blocks) next to rank 1's value-indexed rows in one
    CG; afterwards rank 0 is latched (vi_declined) and rank 1 is not."""
    long = check_two_ranks("one_rank_overflows")
    assert [s["info"]["storage"] == 3 for s in long[0]] == [True, False, False]
    assert [s["info"]["storage"] == 3 for s in long[1]] == [True, True, True]


# ---------------------------------------------------------------- multigrid
def test_multigrid_hierarchy_follows():
    """-pc_type mg on 17^3 (three levels), one -> one moved -> none: every assembly_jac drops the
    hierarchy; pc_apply, pc_mg_info and the solve equal a fresh context's bit for bit."""
    grid = "g17"
    argv = R.argv(grid, "-pc_type", "mg")

    def snap(m, r):
        z = m.pc_apply(r)
        info = m.pc_mg_info()
        its, rn, reason = m.solve_Ax()
        return z, info, its, rn, reason, m.du()

    refs = R.references(grid, [step.state for step in R.MG_SEQUENCE.steps])
    with M.Macroc(argv) as m:
        for q, step in enumerate(R.MG_SEQUENCE.steps):
            ref = refs[step.state]
            assemble(m, ref.u)
            assert m.get_info()["vi_exc_nodes"] == ref.nexc and m.get_info()["storage"] == 3
            assert np.array_equal(m.dump_csr()[2], ref.v)
            z, info, its, rn, reason, du = snap(m, ref.x)
            with M.Macroc(argv) as f:
                assemble(f, ref.u)
                fz, finfo, fits, frn, freason, fdu = snap(f, ref.x)
            print(f"mg step {q} {step.state}: levels {info['levels']} lmax {info['lmax']} its {its} reason {reason}")
            assert info["levels"] == 3 and np.any(z != 0)
            assert np.array_equal(z, fz)
            assert info["levels"] == finfo["levels"] and np.array_equal(info["nxyz"], finfo["nxyz"])
            assert np.array_equal(info["lmax"], finfo["lmax"]) and info["bytes"] == finfo["bytes"]
            assert (its, rn, reason) == (fits, frn, freason) and np.array_equal(du, fdu)
