"""-mat_law micro_nl, the checks that need no GPU: the flag parses to a law of its own, the new
entries are exported and declared, the ABI revision is unchanged, and the entries fail cleanly
without a context."""
import ctypes as C
import os
import re

import pytest

import macroc_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mcx_get_gp_ctan", "mcx_micro_nl_get_info", "mcx_micro_nl_get_pool")


def test_mat_law_micro_nl_parses_to_its_own_law():
    o = M.parse_args(["-mat_law", "micro_nl", "-micro_n", "5", "-micro_type", "0", "-micro_mat_1", "1e7,0.25,1e4,1e6",
                      "-micro_mat_2", "1e8,0.3,1e9,1e7"])
    assert o.mat_law == 4 == M.LAWS["micro_nl"]
    assert (o.micro_n, o.micro_type) == (5, 0)
    assert list(o.micro_mat_1) == [1e7, 0.25, 1e4, 1e6] and list(o.micro_mat_2) == [1e8, 0.3, 1e9, 1e7]
    # the other laws keep their numbers
    assert [M.parse_args(["-mat_law", k]).mat_law for k in ("elastic", "plastic", "external", "micro")] == [0, 1, 2, 3]


@pytest.mark.parametrize("bad", ["micro_n", "micro_nl2", "MICRO_NL", "micro-nl"])
def test_near_misses_are_refused_and_the_message_lists_the_law(bad):
    with pytest.raises(M.MacrocError, match="micro_nl, elastic, plastic, external or micro, got " + bad):
        M.parse_args(["-mat_law", bad])


def test_entries_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "macroc_amd.h")).read()
    for sym in NEW:
        assert sym in M.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr)
        getattr(M.lib(), sym)
    assert re.search(r"MCX_LAW_MICRO_NL\s*=\s*4", hdr)
    for opt in ("micro_nl_rtol", "micro_nl_max_it", "micro_nl_slots"):
        assert opt in hdr
    assert hasattr(M.Macroc, "gp_ctan") and hasattr(M.Macroc, "micro_nl_info")


def test_abi_version_unchanged():
    assert M.lib().mcx_abi_version() == 3 == M.ABI_VERSION


def test_entries_refuse_a_null_context():
    L = M.lib()
    buf = (C.c_double * 36)()
    assert L.mcx_get_gp_ctan(None, buf) != 0
    assert L.mcx_micro_nl_get_info(None, None, None, None, None) != 0
    assert L.mcx_micro_nl_get_pool(None, None, None, None) != 0
    assert L.mcx_last_error()  # a message, not a crash
