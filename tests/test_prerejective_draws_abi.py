"""CPU-side checks of include/ope_device_draws.h (the device draws of the batched prerejective aligner): ope.h includes it, its
entries are declared, exported and bound from a table of their own with the header's arity, and it declares no struct."""
import ctypes
import os
import re

import pytest

from conftest import ROOT, load_pkg

OPE_H = os.path.join(ROOT, "include", "ope.h")
HEADER = os.path.join(ROOT, "include", "ope_device_draws.h")
ENTRIES = {"ope_prerejective_set_draws": 2, "ope_prerejective_get_draws": 2, "ope_prerejective_set_draws_limits": 3,
           "ope_prerejective_draws_device": 12,
           "ope_prerejective_draws_last_stats": 2}


def source(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


@pytest.fixture(scope="module")
def ope():
    pkg = load_pkg()
    pkg.build_library()
    return pkg


def test_ope_h_includes_the_header_inside_its_extern_c_block():
    src = source(OPE_H)
    at = src.index('#include "ope_device_draws.h"')
    assert src.index('#include "ope_batch_rejectors.h"') < at < src.rindex("#ifdef __cplusplus")
    assert "#error" in source(HEADER) and "OPE_H" in source(HEADER)          # not to be included alone


def test_header_declares_exactly_the_entries_and_no_struct():
    src = source(HEADER)
    decls = re.findall(r"([\w \t*]+?)\b(ope_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src)
    assert sorted(name for _, name, _ in decls) == sorted(ENTRIES)
    for ret, name, params in decls:
        assert ret.strip() == "int" and len(params.split(",")) == ENTRIES[name], name
    assert "typedef" not in src and "struct" not in src
    assert re.search(r"OPE_DRAWS_HOST\s*=\s*0\b", src) and re.search(r"OPE_DRAWS_DEVICE\s*=\s*1\b", src)


def test_entries_are_exported_and_bound_from_their_own_table(ope):
    L = ctypes.CDLL(ope.LIB_PATH)
    table = {name: (res, args) for name, res, args in ope.ABI_DEVICE_DRAWS}
    assert sorted(table) == sorted(ENTRIES)
    assert not set(ENTRIES) & {name for name, _, _ in ope.ABI}
    assert not set(ENTRIES) & {name for name, _, _ in ope.ABI_BATCH_REJECTORS}
    for name, arity in ENTRIES.items():
        assert hasattr(L, name), name
        res, args = table[name]
        assert res is ctypes.c_int and len(args) == arity, name
        fn = getattr(ope.lib(), name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == list(args), name
    assert (ope.DRAWS_HOST, ope.DRAWS_DEVICE) == (0, 1)
    assert len(ope.DRAWS_STATS_FIELDS) == 8
    for method in ("prerejective_set_draws", "prerejective_get_draws", "prerejective_set_draws_limits", "prerejective_draws_device", "prerejective_draws_stats"):
        assert callable(getattr(ope.Context, method))
    assert L.ope_abi_version() == 5                                          # the change only adds to the ABI


def test_null_context_is_refused_without_a_device(ope):
    L = ope.lib()
    out = (ctypes.c_int64 * 8)()
    mode = ctypes.c_int(7)
    assert L.ope_prerejective_set_draws(None, 1) == ope.OPE_EINVAL
    assert L.ope_prerejective_set_draws_limits(None, 0, 0) == ope.OPE_EINVAL
    assert L.ope_prerejective_get_draws(None, ctypes.byref(mode)) == ope.OPE_EINVAL and mode.value == 7
    assert L.ope_prerejective_draws_last_stats(None, out) == ope.OPE_EINVAL
    assert L.ope_prerejective_draws_device(None, 10, 3, 1, 1, None, 1, 0, 0, None, None, None) == ope.OPE_EINVAL
