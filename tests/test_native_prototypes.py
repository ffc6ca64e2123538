"""topolow_amd/_native.py against include/topolow_relax.h, mechanically: every prototype of _native.PROTOTYPES type by
type, every constant the two share, and size, field names and field offsets of every ctypes twin of a header struct.
Host only: the header is parsed as text, the structs are measured by a C program compiled against it."""
import ctypes as C
import os
import re
import subprocess

from topolow_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCALARS = {"int": C.c_int, "int8_t": C.c_int8, "uint8_t": C.c_uint8, "int32_t": C.c_int32, "uint32_t": C.c_uint32,
           "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
OPAQUE = ("void", "topolow_session", "topolow_layout_prep")   # the binding never looks behind a pointer to these


def _header() -> str:
    text = open(os.path.join(ROOT, "include", "topolow_relax.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def _twin(c_name: str):
    """topolow_run_stats -> _native.TopolowRunStats"""
    return getattr(_native, "".join(word.capitalize() for word in c_name.split("_")))


def _ctype(text: str):
    """The ctypes type of a C type as the header spells it: `const` and `struct` dropped, a pointer to an opaque type
    is c_void_p, `char*` is c_char_p, topolow_<struct> is its ctypes twin, every further `*` a POINTER."""
    text = "".join(re.sub(r"\b(const|struct)\b", "", text).split())
    base, stars = text.rstrip("*"), len(text) - len(text.rstrip("*"))
    if base in OPAQUE or base == "char":
        assert stars >= 1, text
        ty, stars = (C.c_char_p if base == "char" else C.c_void_p), stars - 1
    else:
        ty = SCALARS[base] if base in SCALARS else _twin(base)
    for _ in range(stars):
        ty = C.POINTER(ty)
    return ty


def _split(params: str):
    """The parameters of a declaration, split at the commas outside parentheses (a function pointer has its own)."""
    out, depth = [""], 0
    for ch in params:
        depth += (ch == "(") - (ch == ")")
        if ch == "," and depth == 0:
            out.append("")
        else:
            out[-1] += ch
    return [" ".join(p.split()) for p in out if p.strip()]


DECLARATION = re.compile(r"^([A-Za-z_][\w \t*]*?)\b(topolow_[a-z0-9_]+)\s*\(((?:[^()]|\([^()]*\))*)\)\s*;", re.M)


def _declarations():
    """[(name, return type text, [(parameter type text or None for a function pointer, parameter name)])]"""
    out = []
    for ret, name, params in DECLARATION.findall(_header()):
        plist = []
        for p in _split(params):
            if p == "void":
                continue
            callback = re.match(r".*\(\s*\*\s*(\w+)\s*\)\s*\(.*\)$", p)
            plist.append((None, callback.group(1)) if callback else re.match(r"(.*?)(\w+)$", p).groups())
        out.append((name, " ".join(ret.split()), plist))
    return out


def test_every_prototype_matches_the_header_type_by_type():
    lib = _native.load()
    decls = _declarations()
    names = [d[0] for d in decls]
    loose = set(re.findall(r"\b(topolow_[a-z0-9_]+)\s*\(", _header()))   # test_library_exports_every_declared_symbol's
    assert len(names) == len(set(names)) and set(names) == loose, set(names) ^ loose
    assert len(names) >= 106
    assert set(_native.PROTOTYPES) == loose, set(_native.PROTOTYPES) ^ loose
    for name, ret, params in decls:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), name
        expected = []
        for (ctext, pname), bound in zip(params, fn.argtypes):
            if ctext is None:
                assert pname == "interrupt_cb", (name, pname)
                expected.append(_native.INTERRUPT_CB)
            elif pname.startswith("d_") and bound is C.c_void_p:
                assert ctext.rstrip().endswith("*"), (name, pname)
                expected.append(C.c_void_p)     # a device address: passed as a Python int, whatever it points to
            else:
                expected.append(_ctype(ctext))
        assert list(fn.argtypes) == expected, (name, [p[1] for p in params], list(fn.argtypes), expected)
        if ret == "void":
            want = None
        elif ret == "const char*":
            want = C.c_char_p
        elif ret.endswith("*"):
            want = C.c_void_p                   # any other pointer comes back as an address
        else:
            want = _ctype(ret)
        assert fn.restype is want, (name, fn.restype, want)


def test_constants_equal_the_header_defines():
    defines = {name: int(value, 0) for name, value in
               re.findall(r"^#define[ \t]+TOPOLOW_(\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$", _header(), re.M)}
    shared = sorted(name for name in defines if hasattr(_native, name))
    for name in shared:
        assert getattr(_native, name) == defines[name], name
    stagings = {name[len("POST_STAGING_"):].lower(): v for name, v in defines.items() if name.startswith("POST_STAGING_")}
    assert stagings == _native.POST_STAGINGS and len(stagings) == 4
    required = {"OK", "PRUNE_MAX_ATTEMPTS", "FIT_IN", "FIT_OUT", "FIT_ALL"}
    required |= {name for name in defines if name.startswith(("ERR_", "SCHEDULE_", "PRECISION_", "ORDER_"))}
    assert required <= set(shared), required - set(shared)
    assert len(required) + len(stagings) >= 27


def _header_structs():
    """{c name: [field names in order]} of every `typedef struct topolow_x { ... } topolow_x;`"""
    out = {}
    for name, body in re.findall(r"typedef\s+struct\s+(topolow_\w+)\s*\{(.*?)\}\s*\1\s*;", _header(), re.S):
        fields = []
        for statement in body.split(";"):
            statement = " ".join(statement.split())
            if not statement:
                continue
            callback = re.match(r".*?\(\s*\*\s*(\w+)\s*\)\s*\(.*\)$", statement)
            if callback:
                fields.append(callback.group(1))
                continue
            for declarator in statement.split(","):      # `int32_t n, ndim, n_iter` and `double seconds[3]`
                fields.append(re.match(r".*?(\w+)\s*(\[[^\]]*\])?$", declarator.strip()).group(1))
        out[name] = fields
    return out


def test_struct_twins_match_the_header_field_by_field(tmp_path):
    structs = _header_structs()
    assert len(structs) == 11, sorted(structs)
    lines, expected = [], []
    for name in structs:
        twin = _twin(name)
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        expected.append("%s %d" % (name, C.sizeof(twin)))
        for f, _ in twin._fields_:       # the twin's own names: a misnamed field does not compile
            lines.append('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (name, f, name, f, name, f))
            expected.append("%s.%s %d %d" % (name, f, getattr(twin, f).offset, getattr(twin, f).size))
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "topolow_relax.h"\nint main(void) {\n'
                   + "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    measured = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert [m for m in measured if m] == expected
    for name, fields in structs.items():
        assert [f for f, _ in _twin(name)._fields_] == fields, name
