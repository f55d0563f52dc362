"""CPU-side checks of the batched ICP entry point (ope_icp_run_batch): declared, exported and bound, and the ctypes
struct of its per-problem result lays out exactly as the C compiler lays out ope_icp_batch_result."""
import ctypes
import os
import re
import subprocess

import pytest

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


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ope.h"
#define F(m) printf("%s %zu\n", #m, offsetof(ope_icp_batch_result, m))
#define R(m) printf("result.%s %zu\n", #m, offsetof(ope_icp_batch_result, result) + offsetof(ope_icp_result, m))
int main(void) {
  printf("sizeof %zu\n", sizeof(ope_icp_batch_result));
  F(result); F(T); F(fitness); F(fitness_n);
  R(iterations); R(converged); R(state); R(last_mse); R(n_corr); R(align_strength);
  return 0;
}
"""


def test_batch_result_layout_matches_the_c_compiler(ope, tmp_path):
    c = tmp_path / "probe.c"
    c.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    want = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    want = {k: int(v) for k, v in want.items()}
    B, R = ope.IcpBatchResult, ope.IcpResult
    got = {"sizeof": ctypes.sizeof(B)}
    for name, _ in B._fields_:
        got[name] = getattr(B, name).offset
    for name, _ in R._fields_:
        got["result." + name] = B.result.offset + getattr(R, name).offset
    assert got == want
