"""CPU-side checks of the batched ICP entry points that take a list of global rejectors (ope_icp_run_batch_rejectors,
ope_final_pose_batch_rejectors): declared, exported and bound with the argument types of the header, following
tests/test_icp_batch_abi.py.  They are declared in include/ope_batch_rejectors.h, which include/ope.h includes, and bound from a
table of their own (ABI_BATCH_REJECTORS) that lib() binds with the rest."""
import ctypes
import os
import re

import pytest

from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "ope_batch_rejectors.h")
MAIN_HEADER = os.path.join(ROOT, "include", "ope.h")
ENTRIES = ("ope_icp_run_batch_rejectors", "ope_final_pose_batch_rejectors")


@pytest.fixture(scope="module")
def ope():
    pkg = load_pkg()
    pkg.build_library()
    return pkg


def declaration(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", ENTRIES)
def test_entry_is_declared_exported_and_bound(ope, name):
    declaration(name)
    assert hasattr(ctypes.CDLL(ope.LIB_PATH), name)
    assert name in {n for n, _, _ in ope.ABI_BATCH_REJECTORS} and name not in {n for n, _, _ in ope.ABI}
    fn = getattr(ope.lib(), name)          # lib() binds the table: the types are on the function
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == list({n: a for n, _, a in ope.ABI_BATCH_REJECTORS}[name])
    assert hasattr(ope.Context, {"ope_icp_run_batch_rejectors": "icp_batch_rejectors",
                                 "ope_final_pose_batch_rejectors": "final_pose_batch_rejectors"}[name])


def test_argument_types_follow_the_header(ope):
    C = ctypes
    vp, fp, ip = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32)
    by_c_type = {
        "ope_ctx *": vp, "const ope_cloud *": vp, "size_t": C.c_size_t, "double": C.c_double, "const float *": fp, "float *": fp,
        "int32_t *": ip, "const ope_cloud *const *": C.POINTER(vp), "const ope_index *const *": C.POINTER(vp),
        "const ope_icp_params *": C.POINTER(ope.IcpParams), "const ope_final_params *": C.POINTER(ope.FinalParams),
        "const ope_global_rejector *": C.POINTER(ope.GlobalRejector), "ope_global_rejector_stats *": C.POINTER(ope.GlobalRejectorStats),
        "ope_icp_batch_result *": C.POINTER(ope.IcpBatchResult), "ope_final_batch_result *": C.POINTER(ope.FinalBatchResult),
        "const uint64_t *": C.POINTER(C.c_uint64),
    }
    bound = {n: (res, args) for n, res, args in ope.ABI_BATCH_REJECTORS}
    assert sorted(bound) == sorted(ENTRIES)          # the table and the header hold the same two
    for name in ENTRIES:
        res, args = bound[name]
        assert res is C.c_int
        want = []
        for a in declaration(name):
            t = re.sub(r"\s*\b\w+$", "", a).strip()          # drop the parameter's name
            t = re.sub(r"\s*\*", " *", t).replace("* *", "**").replace("*const", "*const ")
            t = " ".join(t.split()).replace("*const *", "*const *")
            assert t in by_c_type, (name, a, t)
            want.append(by_c_type[t])
        assert list(args) == want, name
    fn = getattr(ope.lib(), "ope_icp_run_batch_rejectors")
    assert list(fn.argtypes) == list(bound["ope_icp_run_batch_rejectors"][1])


def test_the_main_header_includes_the_declarations():
    """A program that includes ope.h alone sees both prototypes: the C compiler is asked."""
    import subprocess
    src = '#include "ope.h"\nint main(void) { return ' + " && ".join(f"(void *){n} != (void *)0" for n in ENTRIES) + " ? 0 : 1; }\n"
    for cc, lang in (("gcc", "c"), ("g++", "c++")):
        r = subprocess.run([cc, "-x", lang, "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-"], input=src,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    text = re.sub(r"/\*.*?\*/", "", open(MAIN_HEADER).read(), flags=re.S)
    assert '#include "ope_batch_rejectors.h"' in text
    declared = set(re.findall(r"\b(ope_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)))
    assert declared == set(ENTRIES)


def test_the_stats_of_the_batch_are_the_struct_of_the_single_path(ope):
    assert [f for f, _ in ope.GlobalRejectorStats._fields_] == ["n_in", "n_out", "threshold", "ratio", "launches"]
    assert ctypes.sizeof(ope.GlobalRejectorStats) == 40 and ctypes.sizeof(ope.GlobalRejector) == 32
