"""The layout of structs as the C compiler sees it (c_layout) and as ctypes sees it (ctypes_layout), in one shape:
{(C type name, field name or "sizeof"): int}.  The C program is written from _fields_, so every field of every struct given is
compared, and a field the ctypes class lacks shows up as a size or a later offset that differs."""
import ctypes
import os
import subprocess
import tempfile

from conftest import ROOT


def c_layout(structs, extra=None):
    """structs: {ctypes class: C type name}.  Compiles, against include/ope.h, a program that prints sizeof of each type and offsetof
    of every name in its class's _fields_, and returns what it prints.  extra: {key: C integer expression} (a macro, an enumerator),
    each returned under its key."""
    body = []
    for S, ctype in structs.items():
        body.append(f'printf("{ctype} sizeof %zu\\n", sizeof({ctype}));')
        body += [f'printf("{ctype} {f[0]} %zu\\n", offsetof({ctype}, {f[0]}));' for f in S._fields_]
    body += [f'printf("{key} %ld\\n", (long)({expr}));' for key, expr in (extra or {}).items()]
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "ope.h"\nint main(void) {\n  ' + "\n  ".join(body) + "\n  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        with open(c, "w") as f:
            f.write(src)
        subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        lines = subprocess.check_output([exe], text=True).splitlines()
    out = {}
    for line in lines:
        *key, value = line.split()
        out[tuple(key) if len(key) == 2 else key[0]] = int(value)
    return out


def ctypes_layout(structs):
    """The same dictionary from ctypes.sizeof and the field descriptors."""
    out = {}
    for S, ctype in structs.items():
        out[(ctype, "sizeof")] = ctypes.sizeof(S)
        for f in S._fields_:
            out[(ctype, f[0])] = getattr(S, f[0]).offset
    return out
