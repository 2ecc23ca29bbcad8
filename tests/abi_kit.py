"""What the ABI tests share: include/tloam_hip.h as gcc sees it (values of C expressions, every struct's layout, every
TLOAM_* constant), as a text (struct bodies, declared functions), and the symbols the built library exports.  Every result is
cached, so a session compiles each distinct C program once; the header's own layout and constants are one program."""
import functools
import os
import re
import subprocess
import tempfile

from tloam_amd import registration as reg

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


@functools.lru_cache(maxsize=None)
def header_text():
    """include/tloam_hip.h, comments stripped"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "tloam_hip.h")).read(), flags=re.S)


@functools.lru_cache(maxsize=None)
def _compile_and_run(exprs):
    lines = "".join(f'  printf("%lld\\n", (long long)({e}));\n' for e in exprs)
    src = f'#include <stdio.h>\n#include <stddef.h>\n#include "tloam_hip.h"\nint main(void) {{\n{lines}  return 0;\n}}\n'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        with open(c, "w") as fh:
            fh.write(src)
        subprocess.check_call(["gcc", "-I", INCLUDE, c, "-o", exe])
        vals = tuple(map(int, subprocess.check_output([exe]).split()))
    assert len(vals) == len(exprs)
    return vals


def c_values(exprs):
    """the integer values of the C expressions `exprs`, in a program that includes tloam_hip.h"""
    return list(_compile_and_run(tuple(exprs)))


@functools.lru_cache(maxsize=None)
def header_structs():
    """{C name: [field names in order]} of every `typedef struct NAME { ... } NAME;` of the header"""
    out = {}
    for name, body in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", header_text(), flags=re.S):
        decls = [d for d in body.split(";") if d.strip()]
        # `type a, b[N]` declares a and b: the last word before any bracket of each comma-separated piece
        out[name] = [re.findall(r"\w+", piece.split("[")[0])[-1] for d in decls for piece in d.split(",")]
    return out


@functools.lru_cache(maxsize=None)
def declared_functions():
    """every function the header declares"""
    return frozenset(re.findall(r"\b(tloam_[a-z0-9_]+)\s*\(", header_text())) - {"tloam_allreduce_fn"}


@functools.lru_cache(maxsize=None)
def _header_values():
    """{expression: value}: sizeof of every struct, offsetof and sizeof of every member, every TLOAM_* constant (macro or
    enumerator) -- one program"""
    exprs = [n for n in sorted(set(re.findall(r"\bTLOAM_[A-Z0-9_]+\b", header_text()))) if n != "TLOAM_HIP_H"]
    for name, fields in header_structs().items():
        exprs.append(f"sizeof({name})")
        for f in fields:
            exprs += [f"offsetof({name}, {f})", f"sizeof((({name}*)0)->{f})"]
    return dict(zip(exprs, c_values(exprs)))


def constants(*names):
    """the values of the header's TLOAM_* constants `names`"""
    return [_header_values()[n] for n in names]


def sizes(*c_names):
    return [_header_values()[f"sizeof({n})"] for n in c_names]


def offsets(c_name):
    """offsetof of every member of the header's struct, in order"""
    return [_header_values()[f"offsetof({c_name}, {f})"] for f in header_structs()[c_name]]


def member_sizes(c_name):
    return [_header_values()[f"sizeof((({c_name}*)0)->{f})"] for f in header_structs()[c_name]]


@functools.lru_cache(maxsize=None)
def exported():
    """the dynamic symbols the built library defines"""
    out = subprocess.check_output(["nm", "-D", "--defined-only", reg.LIB_PATH], text=True)
    return frozenset(line.split()[-1] for line in out.splitlines() if line.strip())


def assert_exported(symbols):
    """a feature's entry points: each in the binding's table, resolved by the loaded library and defined in the file"""
    L = reg.load_library()
    for name in symbols:
        assert name in reg.EXPORTED_SYMBOLS
        getattr(L, name)
    assert set(symbols) <= exported()
