"""k_spmv_st_dma (option vi_st_dma): the default-stencil march with direct-to-LDS staging on a 5-slot
x ring computes bitwise the rows and p.w partials of k_spmv_st, and runs only where it is eligible
(even padded row pitch, k_spmv_st's default form).  The padded layout (MCX_PAD_ALIGN, read when a
context is created) decides the pitch and x's alignment: by default the pitch is a multiple of 16
nodes and x is 8 mod 16 bytes (the staged rows are shifted by one double), with 0 the pitch is
nx + 2 and x is 16-byte aligned."""
import numpy as np
import pytest

import macroc_amd as M

pytestmark = pytest.mark.gpu


def argv_for(NX, NY, NZ, rtol, extra=()):
    return ["-da_grid_x", NX, "-da_grid_y", NY, "-da_grid_z", NZ, "-ksp_rtol", repr(rtol), *extra]


def assembled(m):
    m.set_option("vi_stage", 1)  # the staged tiles (at these sizes the default rule chunks z finer)
    m.set_option("vi_st", 1)     # (by default from 2^23 nodes)
    for ts in (0, 1):
        m.apply_bc_on_u(m.get_displacement(ts))
    m.set_strains(); m.homogenize(); m.assembly_res(); m.assembly_jac()


# 48^3: even pitch, a partial x tile; 70 x 20 x 12: two x tiles, the second 6 nodes wide, a partial y
# tile; 38 x 22 x 9: an odd plane count against the two-plane steps, partial tiles; 37^3: odd nx under
# the rounded pitch (48 nodes); 48^3 in the unrounded layout (pitch 50, x 16-byte aligned: no shift)
@pytest.mark.parametrize("grid,pad", [((48, 48, 48), None), ((70, 20, 12), None), ((38, 22, 9), None),
                                      ((37, 37, 37), None), ((48, 48, 48), 0)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"pad{v}")
def test_st_dma_spmv_bitwise(grid, pad, monkeypatch):
    if pad is not None:
        monkeypatch.setenv("MCX_PAD_ALIGN", str(pad))
    with M.Macroc(argv_for(*grid, 1e-12)) as m:
        assembled(m)
        x = np.random.default_rng(5).uniform(-1, 1, m.n)
        for zblocks in (0, 1, 5):
            m.set_option("spmv_zblocks", zblocks)
            m.set_option("vi_st_dma", 1)
            y = m.spmv(x)
            assert m.get_info()["st_dma"] == 1, zblocks
            m.set_option("vi_st_dma", 0)
            y0 = m.spmv(x)
            assert m.get_info()["st_dma"] == 0, zblocks
            assert np.array_equal(y, y0), zblocks
            m.set_option("vi_st", 0)
            assert np.array_equal(y, m.spmv(x)), zblocks
            assert m.get_info()["st_dma"] == 0
            m.set_option("vi_st", 1)
            m.set_option("vi_st_dma", -1)  # the default: on where eligible
            assert np.array_equal(y, m.spmv(x)) and m.get_info()["st_dma"] == 1, zblocks


def test_st_dma_odd_pitch_falls_back(monkeypatch):
    """37^3 in the unrounded layout: the padded row pitch is 39 nodes, odd rows would start 8 mod 16
    bytes and a lane's 16 bytes would straddle rows: k_spmv_st runs whatever vi_st_dma says."""
    monkeypatch.setenv("MCX_PAD_ALIGN", "0")
    with M.Macroc(argv_for(37, 37, 37, 1e-12)) as m:
        assembled(m)
        x = np.random.default_rng(5).uniform(-1, 1, m.n)
        m.set_option("vi_st_dma", 0)
        y0 = m.spmv(x)
        m.set_option("vi_st_dma", 1)
        y = m.spmv(x)
        assert m.get_info()["st_dma"] == 0 and m.get_info()["st_listed"] >= 0
        assert np.array_equal(y, y0)
        with pytest.raises(M.MacrocError):
            m.set_option("vi_st_dma", 2)


@pytest.mark.parametrize("maxits", [0, 5, 6])
def test_st_dma_cg_bitwise(maxits):
    """The CG solve (the march's p.w partials feed alpha): converged, and stopped after an odd and an
    even number of iterations, (its, reason, du) bitwise equal with vi_st_dma 0 and 1."""
    argv = argv_for(70, 20, 12, 1e-12) + (["-ksp_max_it", maxits] if maxits else [])
    out = []
    with M.Macroc(argv) as m:
        assembled(m)
        for dma in (0, 1, 0):
            m.set_option("vi_st_dma", dma)
            its, rn, reason = m.solve_Ax()
            assert m.get_info()["st_dma"] == dma
            out.append((its, reason, m.du()))
    for its, reason, du in out[1:]:
        assert (its, reason) == out[0][:2] and np.array_equal(du, out[0][2])
    if maxits:
        assert out[0][:2] == (maxits, -3)
    else:
        assert out[0][1] > 0


def test_st_dma_multirank_bitwise():
    """Two ranks in one process (516 x 5 x 4 split in x: local boxes 258 wide, even pitch, an internal
    x face at a partial tile's last lane): every rank's y bitwise the same with vi_st_dma 0 / 1 and
    with the per-node index path (vi_st 0)."""
    from test_gpu_multirank import run_group

    NX, NY, NZ = 516, 5, 4
    argv = ["-da_grid_x", NX, "-da_grid_y", NY, "-da_grid_z", NZ, "-da_processors_x", 2, "-da_processors_y", 1,
            "-da_processors_z", 1, "-ksp_rtol", repr(1e-12)]
    xg = np.random.default_rng(29).uniform(-1, 1, 3 * NX * NY * NZ)

    def fn(m):
        m.set_option("vi_stage", 1)
        petsc, nat = m.owned_dofs()
        m.apply_bc_on_u(m.get_displacement(0))
        m.apply_bc_on_u(m.get_displacement(1))
        m.set_strains(); m.homogenize(); m.assembly_res(); m.assembly_jac()
        ys, on = {}, {}
        for st, dma in ((0, 0), (1, 0), (1, 1)):
            m.set_option("vi_st", st)
            m.set_option("vi_st_dma", dma)
            ys[st, dma] = m.spmv(xg[nat])
            on[st, dma] = m.get_info()["st_dma"]
        return dict(ys=ys, on=on, nx=m.get_info()["nx"], listed=m.get_info()["st_listed"])

    for o in run_group(argv, 2, fn):
        assert o["nx"] == 258 and o["listed"] >= 0, o["nx"]
        assert o["on"] == {(0, 0): 0, (1, 0): 0, (1, 1): 1}, o["on"]
        assert np.array_equal(o["ys"][1, 1], o["ys"][1, 0])
        assert np.array_equal(o["ys"][1, 1], o["ys"][0, 0])
