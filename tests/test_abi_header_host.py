"""include/n3d.h against its hand-written restatements, checked with a C compiler and no device.

The header is the documented integration boundary, yet every other test reaches the library through
nas_3d_unet_amd/_lib.py, which restates each prototype, each struct and the flag values by hand; a dozen limits are restated in
the host modules, each tagged `# N3D_<NAME>`.  This file is the only consumer of the header itself:

  hygiene      n3d.h alone is valid C11 and valid C++17 under -Wall -Wextra -Werror -pedantic.
  structs      every `typedef struct n3d_* {..} n3d_*;` is parsed (nested structs, 1-D / 2-D arrays with macro extents, several
               declarators per declaration, comments); a generated C program prints sizeof / offsetof / field size as the compiler
               lays them out; the ctypes twin must have the same field names in the same order at the same offsets with the same
               sizes and the same total size.  STRUCT_TWINS is the whole table: a struct on either side that is not in it fails.
  prototypes   every declared function against _lib.PROTOTYPES: return kind and argument kinds in order (pointer, int / int32_t,
               int64_t, size_t / uint64_t -- one class in ctypes on LP64 --, uint32_t, float, double, void), and where ctypes
               names a struct pointer the header must name that struct.  Any other parameter type (bool, long, char by value..)
               is refused: libffi would pass it "somehow".
  constants    every object-like N3D_* macro that is an integer constant expression is printed by the same probe; the tagged
               module-level constants of nas_3d_unet_amd/*.py must equal them (a tuple-valued constant restates a count: its
               length is compared); a tag that names no macro fails; the flags of _lib.py must all carry a tag.
  documents    the fenced C blocks of INTEGRATION.md section 3 compile against the header; the ctypes stub of that section
               assigns the argtypes / restype / _fields_ that _lib.py has.

All comparisons are exact.  No compiler (neither ROCm's clang nor `cc`) is a FAILURE, not a skip.

Found when written: nothing wrong in the tree -- 20 structs (203 fields), 157 prototypes and 81 integer macros (56 tagged Python
constants) agree.  Six flag lines and the lesion-wise / clean-up record constants carried no tag (or a wildcard one,
`N3D_SEG_REC_*`) and got one; `_lib.LIB_PATH`'s comment began with the environment variable's name and read as a tag for a macro
that does not exist: reworded.  The three hand-written `sizeof` assertions of the older host tests also state kernel-argument
budgets (`8 * sizeof + 64 <= 4096`), which this file does not, so they stay where they are.

Mutation evidence (each applied alone to a scratch copy of the tree, then this file run there):
  * `double* sums; int32_t rows;` of n3d_gn_bwd_term -> `int32_t rows; double* sums;` (header only)
        -> test_struct_layout_parity[n3d_gn_bwd_term] fails (field names / order), the other 26 tests pass.
  * `"n3d_stats_rows": (_i, [_i64, _i])` -> `[_i, _i]` in PROTOTYPES
        -> test_prototype_parity fails naming n3d_stats_rows argument 0 (header i64, ctypes i32).
  * `#define N3D_PATCH_AUG_MAX_BATCH 32` -> 24 (header only)
        -> test_constant_parity fails naming generator.AUG_MAX_BATCH.
  * `int n3d_zero(void* p, size_t bytes, void* stream)` -> `(void* p, size_t bytes, bool zero_all, void* stream)`, <stdbool.h> included
        -> test_prototype_parity fails: "n3d_zero argument 2: 'bool' is not an ABI kind this binding passes".
Not shown: a header that is valid C++ but not C through an implicit `typedef` (struct tag used without `struct`) -- no struct of
the header refers to another by tag, so the mutation has nothing to act on; the hygiene test would catch it by construction.
"""
import ast
import ctypes as C
import importlib
import io
import os
import re
import shutil
import subprocess
import tokenize
import types

import pytest

from nas_3d_unet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "n3d.h")
INTEGRATION = os.path.join(ROOT, "INTEGRATION.md")

# header struct -> ctypes twin: the whole table, both ways
STRUCT_TWINS = {
    "n3d_conv_geom": "ConvGeom", "n3d_pack_job": "PackJob", "n3d_final_job": "FinalJob", "n3d_conv_fwd_call": "ConvFwdCall",
    "n3d_dw_job": "DwJob", "n3d_conv_bwd_call": "ConvBwdCall", "n3d_gn_fwd_term": "GnFwdTerm", "n3d_gn_bwd_term": "GnBwdTerm",
    "n3d_plain_coef_term": "PlainCoefTerm", "n3d_se_term": "SeTerm", "n3d_head": "Head", "n3d_loss": "Loss",
    "n3d_patch_desc": "PatchDesc", "n3d_patch_volume": "PatchVolume", "n3d_patch_gdesc": "GatherDesc", "n3d_patch_adesc": "AugDesc",
    "n3d_patch_wdesc": "WarpDesc", "n3d_patch_edesc": "ElasticDesc", "n3d_appear_desc": "AppearDesc", "n3d_stitch_entry": "StitchEntry",
}
# every flag of _lib.py must be among the tagged constants
LIB_FLAGS = ("RELU_IN", "RELU", "ACCUMULATE", "POOL_MAX", "NO_MFMA", "PREPACKED", "F32", "BF16", "U8", "PATCH_INCLUSIVE", "PATCH_T_U8",
             "SRC_BF16", "DST_BF16", "ACT_BF16", "NO_POINTWISE", "MM_BF16")
SCALAR_KINDS = {"int": "i32", "int32_t": "i32", "int64_t": "i64", "size_t": "u64", "uint64_t": "u64", "uint32_t": "u32",
                "float": "f32", "double": "f64"}


def _compiler():
    rocm = os.environ.get("ROCM_PATH") or "/opt/rocm"
    for cand in (os.path.join(rocm, "lib", "llvm", "bin", "clang"), shutil.which("cc")):
        if cand and os.path.exists(cand):
            return cand
    pytest.fail("no C compiler: neither $ROCM_PATH/lib/llvm/bin/clang nor cc exists")


def _run(cmd, **kw):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120, **kw)
    return r.returncode, r.stdout


# ---- the header, parsed

def _parse_header(text):
    """(macros {name: body}, structs {name: [field names]} in order, functions {name: (return type, [argument types])})"""
    macros = {}
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(N3D_\w+)(\(?)(.*)$", text, flags=re.M):
        body = re.sub(r"/\*.*?\*/|//.*", "", m.group(3)).strip()
        if not m.group(2) and body:      # object-like and not an include guard
            macros[m.group(1)] = body
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    code = re.sub(r"//[^\n]*", " ", code)
    code = re.sub(r"^[ \t]*#.*$", " ", code, flags=re.M)
    code = re.sub(r'extern\s+"C"\s*\{', " ", code)
    structs = {}

    def take_struct(m):
        tag, body, name = m.group(1), m.group(2), m.group(3)
        assert tag == name, "typedef struct %s {..} %s: tag and name differ" % (tag, name)
        assert name not in structs, "struct %s defined twice" % name
        assert "{" not in body, "struct %s: an anonymous nested aggregate; the parser wants named structs" % name
        fields = []
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            parts = [p.strip() for p in decl.split(",")]
            first = re.match(r"^(.*?[\s\*])(\w+)((?:\s*\[[^\]]*\])*)$", parts[0])
            assert first and first.group(1).strip(), "struct %s: cannot parse %r" % (name, decl)
            fields.append(first.group(2))
            for p in parts[1:]:
                more = re.match(r"^\**\s*(\w+)((?:\s*\[[^\]]*\])*)$", p)
                assert more, "struct %s: cannot parse declarator %r of %r" % (name, p, decl)
                fields.append(more.group(1))
        structs[name] = fields
        return " "

    code = re.sub(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", take_struct, code, flags=re.S)
    assert "struct" not in code, "a struct the parser did not take: %r" % code[code.index("struct") - 40:code.index("struct") + 80]
    functions = {}
    for stmt in code.split(";"):
        stmt = " ".join(stmt.split())
        if stmt in ("", "}"):
            continue
        m = re.match(r"^(.*?)\b(\w+)\s*\((.*)\)$", stmt)
        assert m, "not a function declaration: %r" % stmt
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        assert name.startswith("n3d_") and name not in functions, "unexpected or repeated declaration %r" % stmt
        assert "(" not in args, "%s: function-pointer parameters are not part of this ABI" % name
        functions[name] = (ret, [] if args in ("", "void") else [a.strip() for a in args.split(",")])
    return macros, structs, functions


def _c_kind(decl, is_param, where):
    """kind of a C return type (is_param False) or parameter declaration: ('ptr', pointee struct or None) / (scalar kind, None)"""
    if "*" in decl or "[" in decl:
        m = re.search(r"\b(n3d_\w+)\s*\*", decl)
        return "ptr", (m.group(1) if m and decl.count("*") == 1 else None)
    toks = [t for t in decl.split() if t != "const"]
    if is_param and len(toks) > 1:
        toks = toks[:-1]           # the parameter's name
    typ = " ".join(toks)
    if typ == "void" and not is_param:
        return "void", None
    assert typ in SCALAR_KINDS, "%s: %r is not an ABI kind this binding passes (pointer, int, int32_t, int64_t, size_t, uint32_t, " \
                                "uint64_t, float, double)" % (where, typ)
    return SCALAR_KINDS[typ], None


def _ct_kind(t, where):
    if t is None:
        return "void", None
    if t in (C.c_void_p, C.c_char_p):
        return "ptr", None
    if isinstance(t, type) and issubclass(t, C._Pointer):
        tgt = t._type_
        return "ptr", (tgt if isinstance(tgt, type) and issubclass(tgt, C.Structure) else None)
    table = {C.c_int32: "i32", C.c_int64: "i64", C.c_uint64: "u64", C.c_size_t: "u64", C.c_uint32: "u32", C.c_float: "f32",
             C.c_double: "f64"}
    assert t in table, "%s: ctypes type %r is not one of the kinds of this ABI" % (where, t)
    return table[t], None


@pytest.fixture(scope="module")
def header():
    return _parse_header(open(HEADER).read())


@pytest.fixture(scope="module")
def probe(header, tmp_path_factory):
    """what the C compiler makes of the header: {'sizeof': {struct: n}, 'fields': {struct: [(name, offset, size)]}, 'macros': {name: v}}"""
    macros, structs, _ = header
    cc, tmp = _compiler(), tmp_path_factory.mktemp("abi_probe")
    # which macros are integer constant expressions: one syntax-only pass, an enum per line, errors name the lines
    lines = ['#include "n3d.h"'] + ["enum { probe_%s = (int)((%s) != 0) };" % (n, n) for n in macros]
    (tmp / "ice.c").write_text("\n".join(lines) + "\n")
    rc, out = _run([cc, "-std=c11", "-fsyntax-only", "-ferror-limit=0", "-I", os.path.dirname(HEADER), str(tmp / "ice.c")])
    names = list(macros)
    bad = {names[int(m.group(1)) - 2] for m in re.finditer(r"ice\.c:(\d+):\d+: error", out)}
    assert rc == 0 or bad, out      # an error outside the enum lines is the header's own
    ints = [n for n in names if n not in bad]
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "n3d.h"', "int main(void) {"]
    for s, fields in structs.items():
        src.append('  printf("S %s %%zu\\n", sizeof(%s));' % (s, s))
        for f in fields:
            src.append('  printf("F %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s, f, s, f, s, f))
    for n in ints:
        src.append('  printf("M %s %%lld\\n", (long long)(%s));' % (n, n))
    src += ["  return 0;", "}"]
    (tmp / "probe.c").write_text("\n".join(src) + "\n")
    rc, out = _run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(tmp / "probe.c"), "-o", str(tmp / "probe")])
    assert rc == 0, out
    rc, out = _run([str(tmp / "probe")])
    assert rc == 0, out
    res = {"sizeof": {}, "fields": {s: [] for s in structs}, "macros": {}}
    for line in out.splitlines():
        w = line.split()
        if w[0] == "S":
            res["sizeof"][w[1]] = int(w[2])
        elif w[0] == "F":
            res["fields"][w[1]].append((w[2], int(w[3]), int(w[4])))
        else:
            res["macros"][w[1]] = int(w[2])
    return res


# ---- hygiene

@pytest.mark.parametrize("lang,std", [("c", "c11"), ("c++", "c++17")])
def test_header_is_clean(lang, std, tmp_path):
    cc = _compiler()
    src = tmp_path / ("only_header." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "n3d.h"\n')
    rc, out = _run([cc, "-x", lang, "-std=" + std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only",
                    "-I", os.path.dirname(HEADER), str(src)])
    assert rc == 0, out


# ---- structs

def _lib_structures():
    return {n: c for n, c in vars(_lib).items() if isinstance(c, type) and issubclass(c, C.Structure) and c is not C.Structure}


def test_struct_table_is_complete(header):
    _, structs, _ = header
    assert set(structs) == set(STRUCT_TWINS), "header structs and STRUCT_TWINS differ: %s" % sorted(set(structs) ^ set(STRUCT_TWINS))
    have = _lib_structures()
    assert set(have) == set(STRUCT_TWINS.values()), "ctypes structures and STRUCT_TWINS differ: %s" % sorted(set(have) ^ set(STRUCT_TWINS.values()))
    assert len(STRUCT_TWINS) == len(set(STRUCT_TWINS.values()))


@pytest.mark.parametrize("name", sorted(STRUCT_TWINS))
def test_struct_layout_parity(name, probe):
    cls = getattr(_lib, STRUCT_TWINS[name])
    c_side = probe["fields"][name]
    py_side = [(f[0], getattr(cls, f[0]).offset, getattr(cls, f[0]).size) for f in cls._fields_]
    assert [f[0] for f in c_side] == [f[0] for f in py_side], "%s: field names / order (header, then _lib.%s)" % (name, cls.__name__)
    assert c_side == py_side, "%s: (name, offset, size) per field: header %s, _lib.%s %s" % (name, c_side, cls.__name__, py_side)
    assert probe["sizeof"][name] == C.sizeof(cls)


# ---- prototypes

def test_prototype_parity(header):
    _, structs, functions = header
    assert len(functions) == len(_lib.PROTOTYPES) >= 157, (len(functions), len(_lib.PROTOTYPES))      # 157 when this test was written
    assert set(functions) == set(_lib.PROTOTYPES), sorted(set(functions) ^ set(_lib.PROTOTYPES))
    twin_of = {getattr(_lib, v): k for k, v in STRUCT_TWINS.items()}
    wrong = []
    for name, (ret, args) in functions.items():
        res, argtypes = _lib.PROTOTYPES[name]
        hk, ck = _c_kind(ret, False, name + " return")[0], _ct_kind(res, name + " return")[0]
        if hk != ck:
            wrong.append("%s returns %s in the header, %s in ctypes" % (name, hk, ck))
        hkinds = [_c_kind(a, True, "%s argument %d" % (name, i)) for i, a in enumerate(args)]
        if len(args) != len(argtypes):
            wrong.append("%s takes %d arguments in the header, %d in ctypes" % (name, len(args), len(argtypes)))
            continue
        for i, (a, t) in enumerate(zip(args, argtypes)):
            (hk, hs), (ck, cs) = hkinds[i], _ct_kind(t, "%s argument %d" % (name, i))
            if hk != ck:
                wrong.append("%s argument %d (%s): header %s, ctypes %s" % (name, i, a, hk, ck))
            elif cs is not None and twin_of[cs] != hs:
                wrong.append("%s argument %d (%s): ctypes points to %s = %s" % (name, i, a, cs.__name__, twin_of[cs]))
    assert not wrong, "\n".join(wrong)


# ---- constants

def _tagged_constants():
    """[(module, python name, macro name)] of every module-level assignment whose comment starts with N3D_ tags"""
    out = []
    pkg = os.path.join(ROOT, "nas_3d_unet_amd")
    for fn in sorted(os.listdir(pkg)):
        if not fn.endswith(".py"):
            continue
        text = open(os.path.join(pkg, fn)).read()
        comments = {}
        for tok in tokenize.generate_tokens(io.StringIO(text).readline):
            if tok.type == tokenize.COMMENT:
                comments[tok.start[0]] = tok.string
        for node in ast.parse(text).body:
            if not isinstance(node, ast.Assign) or len(node.targets) != 1:
                continue
            tgt = node.targets[0]
            elts = tgt.elts if isinstance(tgt, ast.Tuple) else [tgt]
            if not all(isinstance(e, ast.Name) for e in elts):
                continue
            for line in range(node.lineno, node.end_lineno + 1):
                m = re.match(r"#\s*(N3D_\w+(?:\s*[/,]\s*N3D_\w+)*)", comments.get(line, ""))
                if m:
                    tags = re.findall(r"N3D_\w+", m.group(1))
                    assert len(tags) == len(elts), "%s:%d: %d names, %d tags" % (fn, line, len(elts), len(tags))
                    out += [(fn[:-3], e.id, t) for e, t in zip(elts, tags)]
    return out


def test_constant_parity(probe):
    macros = probe["macros"]
    assert len(macros) >= 60 and macros["N3D_OK"] == 0 and macros["N3D_ERR_WORKSPACE"] == -4 and macros["N3D_LW_REC_WORDS"] == 1752
    tagged = _tagged_constants()
    wrong = []
    for mod, name, tag in tagged:
        if tag not in macros:
            wrong.append("%s.%s: tag %s names no integer macro of n3d.h" % (mod, name, tag))
            continue
        v = getattr(importlib.import_module("nas_3d_unet_amd." + mod), name)
        if isinstance(v, (tuple, list)):
            v = len(v)
        if isinstance(v, bool) or not isinstance(v, int) or v != macros[tag]:
            wrong.append("%s.%s = %r, %s = %d" % (mod, name, v, tag, macros[tag]))
    assert not wrong, "\n".join(wrong)
    flags = {n: t for m, n, t in tagged if m == "_lib"}
    assert set(LIB_FLAGS) <= set(flags), "untagged flags in _lib.py: %s" % sorted(set(LIB_FLAGS) - set(flags))
    assert all(flags[n] == "N3D_" + n for n in LIB_FLAGS)
    # the restatements known when this test was written stay tagged
    seen = {(m, n) for m, n, _ in tagged}
    for want in [("postprocess", "REC_WORDS"), ("postprocess", "REC_PACKED"), ("metrics", "LW_MAX_LESIONS"), ("metrics", "LW_REC_WORDS"),
                 ("metrics", "REC_BBOX"), ("metrics", "INF"), ("generator", "AUG_MAX_BATCH"), ("elastic", "MAX_CELLS"),
                 ("appearance", "MAX_RADIUS"), ("preprocess", "REC_WORDS"), ("kernels", "MAX_GROUP_TERMS"), ("kernels", "MAX_REDUCE_TERMS")]:
        assert want in seen, "%s.%s lost its N3D_ tag" % want


# ---- documents

def _section3():
    text = open(INTEGRATION).read()
    return text[text.index("## 3. The C ABI"):text.index("## 4. ")]


DOC_PRELUDE = """#include <stdint.h>
#include <stddef.h>
#include "n3d.h"
void doc_block_%d(uint32_t* sync, void* main, void* side, float* param, const float* grad, float* m, float* v, int64_t n, float lr,
                 const float* lr_dev, int32_t* step, float* loss_dev, void* host_word) {
%s
}
"""


def test_integration_c_blocks_compile(tmp_path):
    blocks = re.findall(r"^```c\n(.*?)^```", _section3(), flags=re.S | re.M)
    assert len(blocks) == 2 and "n3d_sync_wait" in blocks[0] and "n3d_adam_step_guarded" in blocks[1]
    cc = _compiler()
    for i, b in enumerate(blocks):
        src = tmp_path / ("doc_block_%d.c" % i)
        src.write_text(DOC_PRELUDE % (i, b))
        rc, out = _run([cc, "-std=c11", "-fsyntax-only", "-Werror", "-I", os.path.dirname(HEADER), str(src)])
        assert rc == 0, out


def _same_ctype(a, b):
    pa, pb = (isinstance(t, type) and issubclass(t, C._Pointer) for t in (a, b))
    if pa and pb and issubclass(a._type_, C.Structure) and issubclass(b._type_, C.Structure):
        return a._type_._fields_ == b._type_._fields_
    return a is b


def test_integration_ctypes_stub_matches_lib():
    blocks = re.findall(r"^```python\n(.*?)^```", _section3(), flags=re.S | re.M)
    assert len(blocks) == 1
    stub = blocks[0][:blocks[0].index("g = ConvGeom(")]
    stub = "\n".join(l for l in stub.splitlines() if not l.startswith("import ") and not l.startswith("lib = "))

    class FakeLib:
        def __getattr__(self, name):
            fn = types.SimpleNamespace()
            setattr(self, name, fn)
            return fn

    ns = {"C": C, "lib": FakeLib()}
    exec(compile(stub, "INTEGRATION.md section 3", "exec"), ns)
    assert ns["ConvGeom"]._fields_ == _lib.ConvGeom._fields_
    bound = {n: f for n, f in vars(ns["lib"]).items()}
    assert set(bound) == {"n3d_conv_workspace_bytes", "n3d_conv_fwd"}
    for name, fn in bound.items():
        res, argtypes = _lib.PROTOTYPES[name]
        assert fn.restype is res, name
        assert len(fn.argtypes) == len(argtypes), name
        for i, (a, b) in enumerate(zip(fn.argtypes, argtypes)):
            assert _same_ctype(a, b), "%s argument %d: the stub says %r, _lib.py %r" % (name, i, a, b)
