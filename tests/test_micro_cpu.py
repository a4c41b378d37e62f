"""-mat_law micro, the checks that need no GPU: the flag parses, the two entries of the micro cell
are exported and declared, and the ABI revision is unchanged (no struct changed)."""
import os
import re

import pytest

import macroc_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mat_law_micro_parses():
    o = M.parse_args(["-mat_law", "micro", "-micro_n", "10", "-micro_type", "0", "-micro_mat_2", "1e8,0.3,1e4,1e7"])
    assert o.mat_law == 3 == M.LAWS["micro"]
    assert (o.micro_n, o.micro_type) == (10, 0) and list(o.micro_mat_2)[:2] == [1e8, 0.3]
    assert M.parse_args(["-mat_law", "elastic"]).mat_law == 0
    assert M.parse_args([]).mat_law == 0


def test_unknown_mat_law_still_raises_and_lists_micro():
    with pytest.raises(M.MacrocError, match="elastic, plastic, external or micro, got foo"):
        M.parse_args(["-mat_law", "foo"])


def test_micro_entries_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "macroc_amd.h")).read()
    for sym in ("mcx_micro_get_ctan", "mcx_micro_get_phase"):
        assert sym in M.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr)
        getattr(M.lib(), sym)
    assert re.search(r"MCX_LAW_MICRO\s*=\s*3", hdr)


def test_abi_version_unchanged():
    assert M.lib().mcx_abi_version() == 3 == M.ABI_VERSION
