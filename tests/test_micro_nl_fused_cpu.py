"""micro_nl_apply (-micro_nl_apply split|fused), the checks that need no GPU: the flag
parses without a warning and touches no mcx_opts field, its word is checked with the flag named (code
2), the new entry mcx_micro_nl_get_apply is exported, declared and refuses a null context, and the ABI
revision stays 3.  mcx_apply_args and the getter's round trip need a context, so a device:
tests/test_gpu_micro_nl_fused.py."""
import ctypes as C
import os
import re

import pytest

import macroc_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-micro_nl_apply", "split"], ["-micro_nl_apply", "fused"],
                                   ["-micro_nl_solver", "grid", "-micro_nl_tangent", "block", "-micro_nl_apply", "fused",
                                    "-micro_nl_ls", "5"]])
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
    o = M.parse_args(["-mat_law", law, "-micro_nl_apply", "fused"])
    assert capfd.readouterr().err == ""
    assert o.mat_law == M.parse_args(["-mat_law", law]).mat_law


def test_near_misses_are_still_reported(capfd):
    capfd.readouterr()
    M.parse_args(["-micro_nl_applys", "fused"])
    assert "-micro_nl_applys" in capfd.readouterr().err


@pytest.mark.parametrize("bad", ["grid", "1", "Fused", "fuse"])
def test_word_is_checked_with_code_2(bad):
    with pytest.raises(M.MacrocError, match="-micro_nl_apply: split or fused, got " + bad + "$"):
        M.parse_args(["-micro_nl_apply", bad])
    argv = (C.c_char_p * 2)(b"-micro_nl_apply", bad.encode())
    o = M.Opts()
    M.lib().mcx_default_opts(C.byref(o))
    assert M.lib().mcx_parse_args(C.byref(o), 2, argv) == 2
    assert M.lib().mcx_last_error().decode() == "-micro_nl_apply: split or fused, got " + bad


def test_entry_is_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "macroc_amd.h")).read()
    assert "mcx_micro_nl_get_apply" in M.EXPORTS and hasattr(M.lib(), "mcx_micro_nl_get_apply")
    assert re.search(r"\bint\s+mcx_micro_nl_get_apply\s*\(void\* ctx, int\* fused, long long\* launches\);", hdr)
    for word in ('"micro_nl_apply"', "-micro_nl_apply split|fused"):
        assert word in hdr, word
    declared = set(re.findall(r"\b(mcx_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(M.EXPORTS) and len(M.EXPORTS) == len(declared)
    assert hasattr(M.Macroc, "micro_nl_apply") and hasattr(M.Macroc, "micro_nl_apply_launches")
    assert M.lib().mcx_abi_version() == 3 == M.ABI_VERSION


def test_entry_refuses_a_null_context():
    fused, count = C.c_int(7), C.c_longlong(9)
    assert M.lib().mcx_micro_nl_get_apply(None, C.byref(fused), C.byref(count)) != 0
    assert fused.value == 7 and count.value == 9
    assert "null context" in M.lib().mcx_last_error().decode()


def test_readme_design_and_driver_list_the_flag():
    assert "-micro_nl_apply" in open(os.path.join(ROOT, "README.md")).read()
    assert "-micro_nl_apply" in open(os.path.join(ROOT, "macroc_amd", "driver", "main.c")).read()
    assert "micro_nl_apply" in open(os.path.join(ROOT, "DESIGN.md")).read()
