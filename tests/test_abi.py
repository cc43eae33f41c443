"""CPU: polyphonicformer_amd/_lib.py, the hand-written ctypes mirror of include/polyhead.h, against the header itself -- every
struct layout and shared constant as a C compiler sees them (one compiled program), every prototype's return and argument classes
against its SIGNATURES row, the exported symbols, and what the example programs link.  A struct, constant or entry point added to
one side only fails here."""
import ast
import ctypes as C
import functools
import glob
import os
import re
import shutil
import subprocess
import tempfile

import helpers as Hh
from polyphonicformer_amd import _lib
from polyphonicformer_amd import build as BLD

HEADER = os.path.join(Hh.REPO, "include", "polyhead.h")
# C expression, then the values it must equal: _lib's copy and what the Python side derives it from or relies on
CONSTANTS = [
    ("sizeof(ph_stage_layout)", 8 * (2 * 13 + 2 * 30) + 8 + 4 + 4),
    ("PH_DECODE_NPARAMS", _lib.PH_DECODE_NPARAMS),
    ("PH_KPACK_COUNT", _lib.PH_KPACK_COUNT, len(_lib.KPACK_PIECES)),
    ("PH_KHEAD_NPARAMS", _lib.PH_KHEAD_NPARAMS),
    ("PH_NPACK_COUNT", _lib.PH_NPACK_COUNT, 3 * _lib.PH_NECK_NCONVS + 2),
    ("PH_NECK_NPARAMS", _lib.PH_NECK_NPARAMS, 3 * _lib.PH_NECK_NCONVS),
    ("PH_NPACK_OUTS_W", _lib.PH_NPACK_OUTS_W),
    ("PH_NPACK_OUTS_GN", _lib.PH_NPACK_OUTS_GN),
    ("PH_NPACK_WP(9)", 27),
    ("PH_NPACK_BETA(9)", 29),
    ("PH_TRACK_MAX_CONVS", _lib.PH_TRACK_MAX_CONVS),
    ("PH_TPACK_COUNT", _lib.PH_TPACK_COUNT, 3 * _lib.PH_TRACK_MAX_CONVS + 4),
    ("PH_TPACK_FC", _lib.PH_TPACK_FC),
    ("PH_TPACK_FC_B", _lib.PH_TPACK_FC_B),
    ("PH_TPACK_EMB", _lib.PH_TPACK_EMB),
    ("PH_TPACK_EMB_B", _lib.PH_TPACK_EMB_B),
    ("PH_TPACK_GAMMA(3)", _lib.PH_TRACK_MAX_CONVS + 3),
    ("PH_TPACK_BETA(3)", 2 * _lib.PH_TRACK_MAX_CONVS + 3),
    ("PH_DTRK_ST_WORDS", _lib.PH_DTRK_ST_WORDS, len(_lib.DTRK_STATUS), 8),
    ("PH_DTRK_OK", _lib.PH_DTRK_OK, 0),
    ("PH_DTRK_EPOOL", _lib.PH_DTRK_EPOOL, 1),
    ("PH_DTRK_EREFUSED", _lib.PH_DTRK_EREFUSED, 2),
    ("PH_DTRK_ECOUNT", _lib.PH_DTRK_ECOUNT, 3),
    ("PH_DVPQ_MAX_THR", _lib.PH_DVPQ_MAX_THR, 8),
    ("PH_SWITCH_COUNT", len(_lib.SWITCHES), 8),
] + [("PH_DTRK_ST_" + n.upper(), i) for i, n in enumerate(_lib.DTRK_STATUS)] + \
    [("PH_SWITCH_" + n.upper(), i) for i, n in enumerate(_lib.SWITCHES)]


@functools.lru_cache(maxsize=None)
def _c_values():
    """{"ph_x": sizeof, "ph_x.field": offsetof, expression: value} of every _lib.STRUCTS entry and CONSTANTS row, printed by one
    program compiled against the header"""
    cc = shutil.which("cc") or shutil.which("gcc") or BLD._hipcc()
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "polyhead.h"', 'int main(void) {']
    for cname, cls in _lib.STRUCTS.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{field} %zu\\n", offsetof({cname}, {field}));' for field, *_ in cls._fields_]
    lines += [f'printf("{expr} %lld\\n", (long long)({expr}));' for expr, *_ in CONSTANTS]
    lines += ['return 0;', '}']
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.c"), "w") as f:
            f.write("\n".join(lines))
        exe = os.path.join(d, "t")
        lang = [] if os.path.basename(cc) in ("cc", "gcc") else ["-x", "c++"]
        subprocess.run([cc] + lang + ["-I", os.path.dirname(HEADER), os.path.join(d, "t.c"), "-o", exe], check=True,
                       capture_output=True, timeout=300)
        out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout
    return {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}


def test_every_structure_has_a_c_name():
    mirrors = [v for v in vars(_lib).values() if isinstance(v, type) and issubclass(v, C.Structure) and v.__module__ == _lib.__name__]
    missing = [m.__name__ for m in mirrors if m not in _lib.STRUCTS.values()]
    assert not missing, f"ctypes.Structure classes of _lib without a _lib.STRUCTS entry: {missing}"
    assert len(set(_lib.STRUCTS.values())) == len(_lib.STRUCTS) == len(mirrors)


def test_structures_are_defined_in_lib_only():
    """a ctypes mirror defined anywhere else in the package escapes the two tests around this one"""
    pkg = os.path.dirname(_lib.__file__)
    stray = []
    for path in sorted(glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True)):
        if os.path.samefile(path, _lib.__file__):
            continue
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if isinstance(node, ast.ClassDef) and any("Structure" in ast.unparse(b) for b in node.bases):
                stray.append(f"{os.path.relpath(path, pkg)}:{node.lineno} class {node.name}")
    assert not stray, f"ctypes.Structure classes outside _lib.py (move them there, with a _lib.STRUCTS entry): {stray}"


def test_struct_layouts_match_the_header():
    c = _c_values()
    for cname, cls in _lib.STRUCTS.items():
        assert c[cname] == C.sizeof(cls), f"sizeof({cname}): C {c[cname]}, {cls.__name__} {C.sizeof(cls)}"
        for field, *_ in cls._fields_:
            key = f"{cname}.{field}"
            assert c[key] == getattr(cls, field).offset, f"offsetof {key}: C {c[key]}, {cls.__name__} {getattr(cls, field).offset}"
    assert (len(_lib.DvpqCfg._fields_), len(_lib.DvpqIO._fields_)) == (6, 8)


def test_constants_match_the_header():
    c = _c_values()
    for expr, *want in CONSTANTS:
        assert [c[expr]] * len(want) == want, f"{expr}: C {c[expr]}, Python {want}"


# ---- prototypes: a regex over a regular header (return type, name, a parenthesis-free argument list, ';'), no C parser
_PROTO = re.compile(r"(?:^|[;}])\s*((?:const\s+)?\w+[\s*]+)(ph_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", re.M)
_SCALARS = {"int": "i32", "int32_t": "i32", "int64_t": "i64", "size_t": "size", "float": "float", "double": "double", "void": "void"}
_CTYPES = {None: "void", C.c_void_p: "ptr", C.c_char_p: "ptr", C.c_int: "i32", C.c_int32: "i32", C.c_int64: "i64", C.c_size_t: "size",
           C.c_float: "float", C.c_double: "double"}


def _c_class(decl, name):
    """class of a C return type or parameter declaration; a parameter's own name, where it has one, is dropped"""
    if "*" in decl or "[" in decl:
        return "ptr"
    words = decl.replace("const", " ").split()
    words = words[:-1] if len(words) > 1 else words
    assert len(words) == 1 and words[0] in _SCALARS, f"{name}: C type outside the known classes in '{decl.strip()}'"
    return _SCALARS[words[0]]


def _ctypes_class(t, name):
    if isinstance(t, type) and issubclass(t, C._Pointer):
        return "ptr"
    assert t in _CTYPES, f"{name}: ctypes type outside the known classes: {t}"
    return _CTYPES[t]


def _prototypes():
    """name -> (return class, [argument classes]) of every ph_* prototype of the header, comments stripped"""
    hdr = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, args in _PROTO.findall(hdr):
        assert name not in out, name
        args = [] if args.strip() in ("", "void") else args.split(",")
        out[name] = (_c_class(ret, name), [_c_class(a, name) for a in args])
    return out


def test_prototypes_match_signatures():
    protos = _prototypes()
    declared = set(re.findall(r"\b(ph_[a-z0-9_]+)\s*\(", open(HEADER).read())) - {"ph_hw_padded", "ph_n_padded"}
    assert set(protos) == declared, set(protos) ^ declared             # the names test_library_exports_every_declared_symbol finds
    assert set(protos) == set(_lib.SIGNATURES), set(protos) ^ set(_lib.SIGNATURES)
    for name, (ret, args) in protos.items():
        res, argtypes = _lib.SIGNATURES[name]
        assert _ctypes_class(res, name) == ret, f"{name}: returns {ret} in the header, {res} in SIGNATURES"
        assert len(argtypes) == len(args), f"{name}: {len(args)} arguments in the header, {len(argtypes)} in SIGNATURES"
        for i, (a, t) in enumerate(zip(args, argtypes)):
            assert _ctypes_class(t, name) == a, f"{name}: argument {i} is {a} in the header, {t} in SIGNATURES"


def test_library_exports_every_declared_symbol():
    from polyphonicformer_amd.build import build_library
    build_library()
    hdr = open(os.path.join(Hh.REPO, "include", "polyhead.h")).read()
    declared = set(re.findall(r"\b(ph_[a-z0-9_]+)\s*\(", hdr)) - {"ph_hw_padded", "ph_n_padded"}
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    lib.ph_version.restype = C.c_int
    assert lib.ph_version() == 100


def test_example_programs_link_no_python():
    """the C++ callers are built next to the library and depend on libpolyhead.so and the HIP runtime only"""
    assert len(BLD.EXAMPLES) >= 3
    for _, prog in BLD.EXAMPLES:
        assert os.path.exists(prog), f"{prog}: built by python -m polyphonicformer_amd.build"
        needed = Hh.elf_needed(prog)
        assert "libpolyhead.so" in needed and any(n.startswith("libamdhip64") for n in needed), (prog, needed)
        assert not any("python" in n or "torch" in n or "c10" in n for n in needed), (prog, needed)
