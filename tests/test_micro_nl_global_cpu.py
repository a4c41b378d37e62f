"""micro_nl_start / micro_nl_ls, the checks that need no GPU: the flags parse without a
warning and touch no mcx_opts field, their words are checked with the flag named, the new entry
mcx_micro_nl_get_steps is exported, declared and refuses a null context, and the ABI revision stays 3."""
import os
import re

import pytest

import macroc_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-micro_nl_start", "zero"], ["-micro_nl_start", "elastic"], ["-micro_nl_ls", "0"],
                                   ["-micro_nl_ls", "5"], ["-micro_nl_ls", "16"],
                                   ["-micro_nl_start", "elastic", "-micro_nl_ls", "5"]])
def test_flags_parse_without_a_warning(flags, capfd):
    base = M.parse_args([])
    capfd.readouterr()
    o = M.parse_args(flags)
    assert capfd.readouterr().err == ""
    for f, _ in M.Opts._fields_:  # the flags' values touch no mcx_opts field
        a, b = getattr(o, f), getattr(base, f)
        assert (list(a) == list(b)) if hasattr(a, "__len__") else (a == b), f
    o = M.parse_args(["-mat_law", "micro_nl", "-micro_n", "12", *flags, "-micro_type", "0"])
    assert capfd.readouterr().err == ""
    assert o.micro_n == 12 and o.micro_type == 0 and o.mat_law == M.parse_args(["-mat_law", "micro_nl"]).mat_law


@pytest.mark.parametrize("law", ["elastic", "plastic", "micro"])
def test_other_laws_accept_the_flags(law, capfd):
    capfd.readouterr()
    o = M.parse_args(["-mat_law", law, "-micro_nl_start", "elastic", "-micro_nl_ls", "3"])
    assert capfd.readouterr().err == ""
    assert o.mat_law == M.parse_args(["-mat_law", law]).mat_law


def test_near_misses_are_still_reported(capfd):
    capfd.readouterr()
    M.parse_args(["-micro_nl_starts", "elastic", "-micro_nl_lss", "3"])
    err = capfd.readouterr().err
    assert "-micro_nl_starts" in err and "-micro_nl_lss" in err


@pytest.mark.parametrize("bad", ["warm", "1", "Elastic"])
def test_start_word_is_checked(bad):
    with pytest.raises(M.MacrocError, match="-micro_nl_start: zero or elastic, got " + bad):
        M.parse_args(["-micro_nl_start", bad])


@pytest.mark.parametrize("bad", ["17", "-1", "2.5", "five", "1e1"])
def test_ls_range_is_checked(bad):
    with pytest.raises(M.MacrocError, match=r"-micro_nl_ls: an integer 0 \.\. 16, got " + re.escape(bad)):
        M.parse_args(["-micro_nl_ls", bad])


def test_entry_is_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "macroc_amd.h")).read()
    assert "mcx_micro_nl_get_steps" in M.EXPORTS and hasattr(M.lib(), "mcx_micro_nl_get_steps")
    assert re.search(r"\bint\s+mcx_micro_nl_get_steps\s*\(void\* ctx, int\* ls_rejects, double\* min_step\);", hdr)
    for word in ("micro_nl_start", "micro_nl_ls", "-micro_nl_start zero|elastic", "-micro_nl_ls K"):
        assert word in hdr, word
    declared = set(re.findall(r"\b(mcx_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(M.EXPORTS) and len(M.EXPORTS) == len(declared)
    assert hasattr(M.Macroc, "micro_nl_steps")
    assert M.lib().mcx_abi_version() == 3 == M.ABI_VERSION


def test_entry_refuses_a_null_context():
    assert M.lib().mcx_micro_nl_get_steps(None, None, None) != 0
    assert "null context" in M.lib().mcx_last_error().decode()
