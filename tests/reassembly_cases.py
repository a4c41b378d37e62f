"""Re-assembly as the exception-node set moves, grows and overflows: the table of hand-placed states
and of the sequences a context lives through.

A plain helper module (no fixtures): tests/test_reassembly_cases_cpu.py proves every state's
preconditions on the CPU oracle, tests/test_gpu_matrix_reassembly.py runs the sequences on the device.

A state is -mat_law plastic (default materials), dt = 0.01, u = 0 except at a set S of nodes, each of
which gets three components uniform(0.05, 0.15) * choice(-1, 1); set_u on both sides, no update_vars,
so no history.  The non-plain elements are then exactly those adjacent to a node of S and the
exception nodes exactly the nodes of those elements (a 3x3x3 cube around an interior node, clipped
at the domain): the set of every state is known in closed form.

Thresholds restated from the library (kernels.hip build_vib, st_auto; mcx_internal.h vi_exc_max):
  capacity  xld grows only when nexc > xld, to min(2 nexc + 1024, nown) rounded up to 64; never shrinks
  st_auto   the default-stencil path on small grids while 0 < nexc <= nown / 10
  overflow  nexc * 1000 > vi_exc_max * nown (300 by default): the next storage (AIJ-split, or blocks)
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

from oracle import oracle as O

DT = 0.01
RTOL = 1e-8
GRIDS = {"g70": (70, 20, 12), "g130": (130, 9, 12), "g17": (17, 17, 17)}
SEQ_GRIDS = ("g70", "g130")   # the sequences' grids; g17 (three multigrid levels) serves MG_SEQUENCE only
ST_FRACTION = 0.10        # st_auto
VI_EXC_MAX = 300          # per mille
# every state sits this far (relative) from the threshold it is meant to be on one side of: the
# nearest is g70's plane_J5 (8.75 % against 10 %); the sets chosen for g130 keep a fifth
MARGIN = {"g70": 0.125, "g130": 0.2, "g17": 0.2}
TWO_RANK_SPLIT_X = 65     # (130, 9, 12) over (2, 1, 1): rank 0 owns x < 65
TWO_RANK_EXC_MAX = 200    # one_rank_overflows: only rank 0's slab exceeds it


def km(grid):
    return GRIDS[grid][2] // 2


def interior_candidates(n3):
    """k_st_setup's five candidate nodes of the interior class, the middle node first."""
    nx, ny, nz = n3
    return [(nx // 2, ny // 2, nz // 2), (2, 2, 2), (nx - 3, ny - 3, nz - 3), (2, ny - 3, nz // 2), (nx - 3, 2, nz // 2)]


def face_candidates(n3, cls):
    """k_st_setup's five candidates of face class cls (1/2 x-lo/x-hi, 3/4 y, 5/6 z): the face's middle
    node and the nodes 2 in from its corners.  The in-face axes are (y, z), (x, z), (x, y)."""
    ax, hi = (cls - 1) >> 1, (cls - 1) & 1
    ua, va = (1 if ax == 0 else 0), (1 if ax == 2 else 2)
    us = [n3[ua] // 2, 2, n3[ua] - 3, 2, n3[ua] - 3]
    vs = [n3[va] // 2, 2, 2, n3[va] - 3, n3[va] - 3]
    out = []
    for u, v in zip(us, vs):
        c = [0, 0, 0]
        c[ax] = n3[ax] - 1 if hi else 0
        c[ua] = max(0, min(n3[ua] - 1, u))
        c[va] = max(0, min(n3[va] - 1, v))
        out.append(tuple(c))
    return out


def class_candidates(n3):
    """The candidate nodes of the seven stencil classes of a (sub)domain of n3 nodes."""
    return [interior_candidates(n3)] + [face_candidates(n3, c) for c in range(1, 7)]


def bump_nodes(grid, name):
    """The set S of a named state, in the order the bumps are drawn."""
    NX, NY, NZ = GRIDS[grid]
    k = km(grid)
    if name == "empty":
        return []
    if name == "one":  # on the 64 x 16 tile corner (g70) / the x tile edge (g130)
        return {"g70": [(64, 16, k)], "g130": [(64, 7, k)], "g17": [(11, 6, k)]}[grid]
    if name == "moved":
        return [(5, 5, 5)]
    if name == "middle":
        return interior_candidates((NX, NY, NZ))[:1]
    if name == "five_interior":
        return interior_candidates((NX, NY, NZ))
    if name == "zlo_face5":
        return face_candidates((NX, NY, NZ), 5)
    if name == "xhi_face5":
        return face_candidates((NX, NY, NZ), 2)
    if name == "plane_J5":  # forces the regrow from `one`'s capacity, at or under 10 %
        if grid == "g70":
            return [(i, j, k) for j in range(1, 6) for i in range(1, NX - 1)]
        return [(i, j, k) for j in range(1, 3) for i in range(1, 91)]
    if name == "plane_half":  # between 10 % and 30 %
        return [(i, j, k) for j in range(1, NY // 2 + 3) for i in range(1, NX - 1)]
    if name == "slab3":  # over 30 %
        return [(i, j, kk) for kk in (k - 1, k, k + 1) for j in range(NY) for i in range(NX)]
    if name == "all":
        return [(i, j, kk) for kk in range(NZ) for j in range(NY) for i in range(NX)]
    if name == "corners":
        return [(0, 0, 0), (NX - 1, NY - 1, NZ - 1)]
    # the two-rank states of g130 (rank boundary between x = 64 and x = 65)
    if name == "straddle":
        return [(65, 4, k)]
    if name == "right":
        return [(100, 4, k)]
    if name == "left":
        return [(20, 4, k)]
    if name == "slab_x55":  # rank 0 over the (lowered) limit, rank 1 with one cube
        return [(i, j, kk) for kk in (k - 1, k, k + 1) for j in range(NY) for i in range(56)] + [(100, 4, k)]
    raise KeyError(name)


# the issue's counts of exception nodes
COUNTS = {
    "g70": {"empty": 0, "one": 27, "moved": 27, "middle": 27, "five_interior": 135, "zlo_face5": 90, "xhi_face5": 90,
            "plane_J5": 1470, "plane_half": 2940, "slab3": 7000, "all": 16800, "corners": 16},
    "g130": {"empty": 0, "one": 27, "moved": 27, "middle": 27, "five_interior": 135, "zlo_face5": 90, "xhi_face5": 90,
             "plane_J5": 1104, "plane_half": 3120, "slab3": 5850, "all": 14040, "corners": 16,
             "straddle": 27, "right": 27, "left": 27, "slab_x55": 57 * 9 * 5 + 27},
    "g17": {"empty": 0, "one": 27, "moved": 27},
}


# The oracle's CG takes 190 to 440 iterations on these states and gains 5 to 10 % per iteration where
# it meets -ksp_rtol, so a solver that sums its dot products in another order (drifting a few per cent
# by then) stops within one iteration of it -- unless the last entries of the history all lie on the
# threshold.  SOLVE_GAP: the entry two before the oracle's last is this far above rtol * h[0]; the
# numpy restatement of the CG (another summation order) must then stop within one iteration too.
# g130's `one` with the plain seed misses it (h / threshold = 1.035, 1.002, 0.947; the restatement
# stops three iterations earlier), and so does slab_x55's (the restatement two later): hence their salts.
SOLVE_GAP = 1.08
SEED_SALT = {("g130", "one"): 2, ("g130", "slab_x55"): 5}


def node_index(grid, i, j, k):
    NX, NY, _ = GRIDS[grid]
    return i + NX * (j + NY * k)


def bump_field(grid, name):
    """u (natural order) of a named state; the seed is the name's, so a state met again is the same bits."""
    NX, NY, NZ = GRIDS[grid]
    salt = SEED_SALT.get((grid, name))
    rng = np.random.default_rng(zlib.crc32((f"{grid}:{name}" + (f":{salt}" if salt else "")).encode()))
    u = np.zeros(3 * NX * NY * NZ)
    for (i, j, k) in bump_nodes(grid, name):
        n = node_index(grid, i, j, k)
        u[3 * n:3 * n + 3] = rng.uniform(0.05, 0.15, 3) * rng.choice([-1.0, 1.0], 3)
    return u


def x_vector(grid, name):
    """The SpMV's input of a state: uniform(-1, 1), a vector of its own per state name.  A state met
    again in a sequence takes the same x: the bit comparisons between the two visits need that."""
    NX, NY, NZ = GRIDS[grid]
    return np.random.default_rng(zlib.crc32(f"x:{grid}:{name}".encode())).uniform(-1, 1, 3 * NX * NY * NZ)


def closed_form_exc(grid, name):
    """Boolean [NZ][NY][NX]: the nodes of the elements adjacent to a node of S = the nodes within one
    grid step of S in every direction, clipped at the domain."""
    NX, NY, NZ = GRIDS[grid]
    s = np.zeros((NZ + 2, NY + 2, NX + 2), dtype=bool)
    for (i, j, k) in bump_nodes(grid, name):
        s[k + 1, j + 1, i + 1] = True
    out = np.zeros((NZ, NY, NX), dtype=bool)
    for dk in range(3):
        for dj in range(3):
            for di in range(3):
                out |= s[dk:dk + NZ, dj:dj + NY, di:di + NX]
    return out


def exc_from_ctan(ct, cref, grid):
    """Host restatement of the exception set from the oracle's Gauss-point tangents (as
    tests/test_gpu_parity.py _exc_waves_per_plane): the nodes of the elements with a tangent other than
    cref (the elastic branch's) at some Gauss point.  Boolean [NZ][NY][NX]."""
    NX, NY, NZ = GRIDS[grid]
    ct = ct.reshape(-1, 8, 36)
    nonplain = np.any(np.any(ct != cref, axis=2), axis=1).reshape(NZ - 1, NY - 1, NX - 1)
    out = np.zeros((NZ, NY, NX), dtype=bool)
    for c in (0, 1):
        for b in (0, 1):
            for a in (0, 1):
                out[c:c + NZ - 1, b:b + NY - 1, a:a + NX - 1] |= nonplain
    return out


def xld_after(xld, nexc, nown):
    """build_vib's capacity rule"""
    if nexc > xld:
        return (min(2 * nexc + 1024, nown) + 63) // 64 * 64
    return xld


def overflows(nexc, nown, exc_max=VI_EXC_MAX):
    return nexc * 1000 > exc_max * nown


def st_auto(nexc, nown):
    return 0 < nexc and nexc * 10 <= nown


# ---------------------------------------------------------------- sequences
# A step: the state assembled, what the long-lived context's storage must be ("vi": 3; "fallback":
# 2 or 0, this assembly overflowed; "latched": although the matrix would fit, the storage the fallback
# step took: vi_declined), an option set before the assembly (name, value; value None = vi_exc_max's
# current value), the state visited earlier in the sequence whose every bit this one must repeat (an
# index, or None), and the storage code where the step fixes it (else None).
Step = namedtuple("Step", "state storage option same_as code", defaults=("vi", None, None, None))
# options: set on the context (and on every fresh one) before the first assembly; exc_max: the
# sequence's vi_exc_max; regrow: the steps whose assembly must grow the capacity
Seq = namedtuple("Seq", "steps options exc_max regrow", defaults=((), VI_EXC_MAX, ()))


def _overflow(big):
    return Seq([Step("one"), Step(big, "fallback"), Step("one", "latched"),
                Step("one", "vi", ("vi_exc_max", None), 0)])


SEQUENCES = {
    # the old site must carry nothing over; the last state repeats the second
    "appear_move_vanish": Seq([Step("empty"), Step("one"), Step("moved"), Step("empty", same_as=0),
                               Step("one", same_as=1)]),
    # the first step forces the capacity regrow; after the shrink the same state runs under the larger xld
    "regrow_shrink": Seq([Step("one"), Step("plane_J5"), Step("one", same_as=0), Step("plane_J5", same_as=1)],
                         regrow=(0, 1)),
    # the default-stencil path on, off, on (vi_st -1)
    "cross_10_percent": Seq([Step("plane_J5"), Step("plane_half"), Step("plane_J5", same_as=0)],
                            options=(("vi_st", -1),)),
    "overflow_and_latch_slab3": _overflow("slab3"),
    "overflow_and_latch_all": _overflow("all"),
    "representatives": Seq([Step("one"), Step("middle"), Step("five_interior"), Step("one", same_as=0)]),
    "face_class_lost_zlo": Seq([Step("one"), Step("zlo_face5"), Step("one", same_as=0)]),
    "face_class_lost_xhi": Seq([Step("one"), Step("xhi_face5"), Step("one", same_as=0)]),
    "corners": Seq([Step("empty"), Step("corners"), Step("empty", same_as=0)]),
    # the context's FIRST default-stencil build finds no interior representative (every class's
    # coefficients zero), the second no z-lo one, the third all seven: nothing of a lost class may stay
    "lost_first": Seq([Step("five_interior"), Step("zlo_face5"), Step("one")]),
    # dense corrections refused (split_dense 0; on these grids every matrix's corrections are dense):
    # the overflow goes to AIJ blocks and split_declined latches with vi_declined; blocks again at
    # `one`; setting split_dense clears split_declined only (AIJ-split, still not value-indexed);
    # setting vi_exc_max clears vi_declined
    "split_refused_and_cleared": Seq([Step("one"), Step("slab3", "fallback", code=0), Step("one", "latched", code=0),
                                      Step("one", "latched", ("split_dense", 1), code=2),
                                      Step("one", "vi", ("vi_exc_max", None), 0)], options=(("split_dense", 0),)),
}

# two ranks, g130 over (2, 1, 1)
SEQUENCES_2R = {
    "straddle_then_one_side": Seq([Step("straddle"), Step("right"), Step("left")]),
    "one_rank_overflows": Seq([Step("one"), Step("slab_x55", "fallback"), Step("one", "latched")],
                              exc_max=TWO_RANK_EXC_MAX),
}
# per state: exception nodes of (rank 0, rank 1)
TWO_RANK_COUNTS = {"straddle": (9, 18), "right": (0, 27), "left": (27, 0), "one": (18, 9),
                   "slab_x55": (57 * 9 * 5, 27)}

# -pc_type mg on g17: the hierarchy is rebuilt after every assembly
MG_SEQUENCE = Seq([Step("one"), Step("moved"), Step("empty")])

# the class whose five candidates a state covers (it loses its representative), the states that cover
# the interior's middle candidate only
CLASS_LOST = {"five_interior": 0, "zlo_face5": 5, "xhi_face5": 2}


# ---------------------------------------------------------------- the oracle
@functools.lru_cache(maxsize=None)
def problem(grid):
    """The oracle's problem of a grid, kept for the module's life and moved by set_u."""
    NX, NY, NZ = GRIDS[grid]
    return O.Problem(NX, NY, NZ, rtol=RTOL, law=1, dt=DT)


def move_oracle(grid, name):
    """The oracle assembled at a named state."""
    P = problem(grid)
    P.set_u(bump_field(grid, name))
    P.set_strains()
    P.homogenize()
    P.assembly_res()
    P.assembly_jac()
    return P


@functools.lru_cache(maxsize=None)
def elastic_ctan(grid):
    """the elastic branch's tangent: every Gauss point's at u = 0"""
    ct = move_oracle(grid, "empty").ctan()
    assert np.all(ct == ct[0])
    return ct[0].copy()


# ---------------------------------------------------------------- the listed rows, restated
@functools.lru_cache(maxsize=None)
def domain_masks(grid):
    """(on[6]: the node is on face class c + 1; nf: faces it is on; near: within one grid step of a
    Dirichlet node, itself included), each boolean / int [NZ][NY][NX]"""
    NX, NY, NZ = GRIDS[grid]
    kk, jj, ii = np.meshgrid(np.arange(NZ), np.arange(NY), np.arange(NX), indexing="ij")
    on = [ii == 0, ii == NX - 1, jj == 0, jj == NY - 1, kk == 0, kk == NZ - 1]
    nf = sum(o.astype(int) for o in on)
    dn = np.unique(problem(grid).dirichlet_set() // 3)
    d = np.zeros((NZ + 2, NY + 2, NX + 2), dtype=bool)
    d[dn // (NX * NY) + 1, (dn // NX) % NY + 1, dn % NX + 1] = True
    near = np.zeros((NZ, NY, NX), dtype=bool)
    for dk in range(3):
        for dj in range(3):
            for di in range(3):
                near |= d[dk:dk + NZ, dj:dj + NY, di:di + NX]
    return on, nf, near


def listed_model(grid, name):
    """k_st_flag restated for one rank on the uniform grid: a node is a listed row of the
    default-stencil SpMV when it is an exception node, on two or three domain faces, on a face whose
    class lost its representative, or when its blocks differ from its class representative's -- which
    here means a Dirichlet row or column was zeroed in them: the node is a Dirichlet node or next to
    one (the representatives are not).  Boolean [NZ][NY][NX]."""
    on, nf, near = domain_masks(grid)
    m = closed_form_exc(grid, name) | (nf > 1) | near
    lost = CLASS_LOST.get(name)
    if lost:
        m = m | (on[lost - 1] & (nf == 1))
    return m


# ---------------------------------------------------------------- references for the device tests
# the oracle at a state, natural order: u, b, the matrix values, the SpMV's input x, y = A x,
# sum |a||x| per row, the closed-form count; its / reason / du of the oracle's solve for the states in
# SOLVED (None elsewhere)
Ref = namedtuple("Ref", "u b v x y absrow nexc its reason du")
# the sequences' last states and every two-rank state: solved by the oracle too
SOLVED = ({q.steps[-1].state for q in SEQUENCES.values()} | {s.state for q in SEQUENCES_2R.values() for s in q.steps})


@functools.lru_cache(maxsize=None)
def pattern(grid):
    return problem(grid).csr()


@functools.lru_cache(maxsize=12)  # 33 MB each on the sequences' grids
def reference(grid, state):
    """The oracle at a state: computed once, shared among the tests, left unchanged."""
    P = move_oracle(grid, state)
    rp, ci = pattern(grid)
    v, x = P.A_values(), x_vector(grid, state)
    its = reason = du = None
    b, y = P.b(), P.spmv(x)
    if state in SOLVED:
        out = P.solve()
        its, reason, du = out["its"], out["reason"], P.du()
    ref = Ref(bump_field(grid, state), b, v, x, y, np.add.reduceat(np.abs(v) * np.abs(x[ci]), rp[:-1]),
              COUNTS[grid][state], its, reason, du)
    for a in ref:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


def references(grid, states):
    """{state: Ref}; call it from the main thread (the oracle's problem of a grid is one object)."""
    return {s: reference(grid, s) for s in dict.fromkeys(states)}


def argv(grid, *more):
    NX, NY, NZ = GRIDS[grid]
    return ["-da_grid_x", NX, "-da_grid_y", NY, "-da_grid_z", NZ, "-dt", DT, "-mat_law", "plastic",
            "-ksp_rtol", repr(RTOL), *more]
