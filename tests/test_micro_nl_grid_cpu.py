"""micro_nl_solver / -micro_nl_solver cell|grid, the checks that need no GPU: the flag parses without
a warning and touches no mcx_opts field, its word is checked, the header documents the option, and
it came without a new entry point or a new ABI revision."""
import os
import re

import pytest

import macroc_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("word", ["grid", "cell"])
def test_flag_parses_without_a_warning(word, capfd):
    base = M.parse_args([])
    capfd.readouterr()
    o = M.parse_args(["-micro_nl_solver", word])
    assert capfd.readouterr().err == ""
    for f, _ in M.Opts._fields_:  # the flag's value touches no mcx_opts field
        a, b = getattr(o, f), getattr(base, f)
        assert (list(a) == list(b)) if hasattr(a, "__len__") else (a == b), f
    o = M.parse_args(["-mat_law", "micro_nl", "-micro_n", "64", "-micro_nl_solver", word, "-micro_type", "0"])
    assert capfd.readouterr().err == ""
    assert o.micro_n == 64 and o.micro_type == 0 and o.mat_law == M.parse_args(["-mat_law", "micro_nl"]).mat_law


def test_near_miss_is_still_reported(capfd):
    capfd.readouterr()
    M.parse_args(["-micro_nl_solvers", "grid"])
    assert "-micro_nl_solvers" in capfd.readouterr().err


@pytest.mark.parametrize("bad", ["hbm", "1", "Grid"])
def test_word_is_checked(bad):
    with pytest.raises(M.MacrocError, match="-micro_nl_solver: cell or grid, got " + bad):
        M.parse_args(["-micro_nl_solver", bad])


def test_header_documents_the_option_and_declares_nothing_new():
    hdr = open(os.path.join(ROOT, "include", "macroc_amd.h")).read()
    assert "micro_nl_solver" in hdr and "-micro_nl_solver cell|grid" in hdr
    declared = set(re.findall(r"\b(mcx_[a-z_0-9]+)\s*\(", hdr))
    assert len(M.EXPORTS) == len(set(M.EXPORTS)) == len(declared)  # no entry was added for the option
    assert declared == set(M.EXPORTS)
    assert not any("solver" in name or "grid" in name for name in declared)
    assert M.lib().mcx_abi_version() == 3 == M.ABI_VERSION
