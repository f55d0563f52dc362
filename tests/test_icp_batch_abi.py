"""CPU-side checks of the batched ICP entry point (ope_icp_run_batch): declared, exported and bound, and the ctypes
struct of its per-problem result lays out exactly as the C compiler lays out ope_icp_batch_result."""
import ctypes
import os
import re

import pytest

from abi_probe import c_layout, ctypes_layout
from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "ope.h")


@pytest.fixture(scope="module")
def ope():
    pkg = load_pkg()
    pkg.build_library()
    return pkg


def test_batch_entry_is_declared_exported_and_bound(ope):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+ope_icp_run_batch\s*\(", src)
    assert hasattr(ctypes.CDLL(ope.LIB_PATH), "ope_icp_run_batch")
    assert "ope_icp_run_batch" in {name for name, _, _ in ope.ABI}


def test_batch_result_layout_matches_the_c_compiler(ope):
    structs = {ope.IcpBatchResult: "ope_icp_batch_result", ope.IcpResult: "ope_icp_result"}
    assert ctypes_layout(structs) == c_layout(structs)
