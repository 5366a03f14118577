"""include/sddp.h as the tests read it, in one place: every prototype, struct and integer #define, the rule by which a ctypes type
binds a C type, and the structs' layout as the C compiler sees it (tests/test_abi.py: the whole of srbd_horizon_amd/_lib.py)."""
import ctypes as C
import os
import re
import subprocess

from srbd_horizon_amd._lib import INCLUDE

HEADER = os.path.join(INCLUDE, "sddp.h")


def text():
    """the header without its comments"""
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def defines():
    """name -> value of every `#define SDDP_* <integer>`; a parenthesised negative such as (-1) counts"""
    return {n: int(v.strip("()")) for n, v in re.findall(r"^#define\s+(SDDP_\w+)\s+(-?\d+|\(-?\d+\))\s*$", text(), flags=re.M)}


def structs():
    """struct name -> [(field, "int" | "double", array length or None)] in the order of declaration"""
    out = {}
    for name, body in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", text(), flags=re.S):
        fields = out[name] = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            base, names = re.fullmatch(r"(int|double)\s+(.*)", decl, flags=re.S).groups()
            for item in names.split(","):
                field, length = re.fullmatch(r"\s*(\w+)\s*(?:\[([\d\s*+()-]+)\])?\s*", item).groups()
                fields.append((field, base, None if length is None else int(eval(length, {"__builtins__": {}}))))
    return out


def _squeeze(decl):
    """one spelling per declaration: single spaces, every * on the type"""
    return re.sub(r"\s*\*\s*", "* ", " ".join(decl.split())).replace("* *", "**").strip()


def functions():
    """name -> (return type, [parameter declarations]) of every sddp_* prototype: ("int", ["sddp_handle* h", "int* on"]); (void): []"""
    src = re.sub(r"typedef\s+struct[^;{]*(\{.*?\})?[^;]*;", " ", re.sub(r"^\s*#.*$", " ", text(), flags=re.M), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(sddp_\w+)\s*\(([^)]*)\)\s*;", src):
        params = [_squeeze(p) for p in params.split(",")]
        out[name] = (_squeeze(ret), [] if params == ["void"] else params)
    return out


_EXACT = {"void": None, "int": C.c_int, "double": C.c_double, "const char*": C.c_char_p, "sddp_handle*": C.c_void_p, "const sddp_handle*": C.c_void_p}
_POINTEES = {"int": C.c_int, "double": C.c_double, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong, "char*": C.c_char_p}


def binds(ctype, ctypes_type, structures):
    """THE rule: may the ctypes type stand for the C type `ctype` (a return type, or a parameter declaration without its name)?
    A scalar int / double binds to exactly c_int / c_double, void (a return type) to None, const char* to c_char_p and sddp_handle*
    to c_void_p.  Any other data pointer T* binds to c_void_p or to POINTER of the type matching T: c_int, c_double, c_longlong,
    c_ulonglong, c_void_p for a pointer (c_char_p for const char*), or the ctypes Structure that `structures` (C struct name ->
    Structure) names; a void* binds to c_void_p alone.  const does not matter otherwise."""
    if ctype in _EXACT or not ctype.endswith("*"):
        return ctype in _EXACT and ctypes_type is _EXACT[ctype]
    pointee = ctype[:-1].replace("const ", "")
    match = _POINTEES.get(pointee) or structures.get(pointee) or (C.c_void_p if pointee.endswith("*") else None)
    return ctypes_type is C.c_void_p or (match is not None and ctypes_type is C.POINTER(match))


def compiled_layout(structures, tmp_path):
    """What gcc makes of the structs (C struct name -> ctypes Structure, whose _fields_ name the members to ask about), by one small
    program on include/sddp.h that links nothing: {"sddp_stats": sizeof, "sddp_stats.cost": (offsetof, sizeof the member), ...}"""
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "sddp.h"', "int main(void) {"]
    for name, S in structures.items():
        lines.append(f'    printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'    printf("{name}.{f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));' for f, *_ in S._fields_]
    src, exe = str(tmp_path / "abi_layout.c"), str(tmp_path / "abi_layout")
    (tmp_path / "abi_layout.c").write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.run(["gcc", "-O0", "-Wall", "-Werror", "-I" + INCLUDE, src, "-o", exe], check=True, capture_output=True)
    rows = (l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    return {r[0]: int(r[1]) if len(r) == 2 else (int(r[1]), int(r[2])) for r in rows}
