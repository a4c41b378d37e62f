"""-pc_type mg without a GPU: the flags parse, the ABI revision and the options struct stay."""
import ctypes as C

import pytest

import macroc_amd as M


def test_parse_args_takes_the_multigrid_flags():
    o = M.parse_args(["-da_grid_x", "17", "-pc_type", "mg", "-pc_mg_levels", "3", "-mg_levels_ksp_max_it", "3",
                      "-pc_mg_galerkin", "-ksp_rtol", "1e-8"])
    assert o.NX == 17 and o.ksp_rtol == 1e-8  # the flags around them are still read
    M.parse_args(["-pc_type", "jacobi"])
    with pytest.raises(M.MacrocError, match=r"only -ksp_type cg / -pc_type jacobi / mg are implemented, got lu"):
        M.parse_args(["-pc_type", "lu"])
    with pytest.raises(M.MacrocError, match="got gmres"):
        M.parse_args(["-ksp_type", "gmres"])


def test_abi_revision_and_opts_layout_unchanged():
    assert M.lib().mcx_abi_version() == 3
    # mcx_opts as of ABI 3: the preconditioner is an option of the context, not a field
    assert C.sizeof(M.Opts) == 264
    o = M.Opts()
    M.lib().mcx_default_opts(C.byref(o))
    assert (o.mat_aij_split, o.mat_aij_vi, o.mat_vi_fma) == (1, 1, 1)  # the last fields are where they were


def test_new_entries_refuse_a_null_context():
    L = M.lib()
    assert L.mcx_pc_apply(None, None, None) != 0
    assert L.mcx_pc_mg_info(None, None, None, None, None) != 0
    assert L.mcx_pc_mg_dump_csr(None, 1, None, None, None) != 0
