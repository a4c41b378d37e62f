"""micro_mem / mcx_apply_args, the checks that need no GPU: the new entry is exported and declared
and fails cleanly without a context, the flags of the cell's solver options parse without a
warning, -micro_mem's word is checked, and neither the ABI revision nor mcx_opts changed."""
import ctypes as C
import os
import re

import pytest

import macroc_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_apply_args_exported_declared_and_refuses_a_null_context():
    hdr = open(os.path.join(ROOT, "include", "macroc_amd.h")).read()
    assert "mcx_apply_args" in M.EXPORTS
    assert re.search(r"\bint\s+mcx_apply_args\s*\(\s*void\s*\*\s*ctx\s*,\s*int\s+argc\s*,\s*const\s+char\s*\*\s*const\s*\*\s*argv\s*\)",
                     hdr)
    assert "micro_mem" in hdr
    L = M.lib()
    argv = (C.c_char_p * 2)(b"-micro_mem", b"device")
    assert L.mcx_apply_args(None, 2, argv) != 0
    assert b"mcx_apply_args" in L.mcx_last_error()  # a message, not a crash


def test_abi_version_unchanged():
    assert M.lib().mcx_abi_version() == 3 == M.ABI_VERSION


def test_solver_flags_parse_without_a_warning(capfd):
    capfd.readouterr()
    o = M.parse_args(["-micro_mem", "device", "-micro_nl_slots", "64"])
    assert capfd.readouterr().err == ""
    assert o.micro_n == 2  # the flags' values touch no mcx_opts field
    M.parse_args(["-micro_mem", "lds", "-micro_rtol", "1e-10", "-micro_max_it", "500", "-micro_nl_rtol", "1e-9",
                  "-micro_nl_max_it", "30", "-micro_n", "12"])
    assert capfd.readouterr().err == ""
    M.parse_args(["-micro_memory", "device"])  # a near miss is still reported as unused
    assert "-micro_memory" in capfd.readouterr().err


@pytest.mark.parametrize("bad", ["hbm", "1", "Device"])
def test_micro_mem_word_is_checked(bad):
    with pytest.raises(M.MacrocError, match="lds or device, got " + bad):
        M.parse_args(["-micro_mem", bad])


def test_opts_did_not_grow():
    """mcx_default_opts fills exactly the Python mirror: bytes past it stay untouched, and the last
    field (mat_vi_fma, default 1) sits at the mirror's end."""
    size = C.sizeof(M.Opts)
    buf = (C.c_ubyte * (size + 64))(*([0xA5] * (size + 64)))
    M.lib().mcx_default_opts(C.cast(buf, C.POINTER(M.Opts)))
    assert all(b == 0xA5 for b in buf[size:])
    o = M.Opts.from_buffer_copy(bytes(buf[:size]))
    assert o.mat_vi_fma == 1 and o.micro_n == 2
    assert size - 8 < M.Opts.mat_vi_fma.offset + 4 <= size  # nothing but tail padding after the last field
    hdr = open(os.path.join(ROOT, "include", "macroc_amd.h")).read()
    body = re.search(r"typedef struct (?:mcx_opts )?\{(.*?)\}\s*mcx_opts;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in re.findall(r"(?:int64_t|int|double)\s+([^;]+);", body) for n in decl.split(",")]
    assert [re.sub(r"\[\d+\]", "", n) for n in names] == [f for f, _ in M.Opts._fields_]
