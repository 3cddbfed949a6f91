"""CPU-side checks of the drop-in boundary: the C-ABI library loads, exports exactly the symbols
include/cpd_hip.h declares, and its host-only entry points behave (no kernels are launched)."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    txt = open(os.path.join(REPO, "include", "cpd_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(cpd_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    from cpd_amd import _lib
    lib = _lib.lib()
    names = declared_functions()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), "libcpd_hip.so does not export %s" % n
        assert n in _lib.SIGNATURES, "python binding lacks %s" % n
    assert sorted(_lib.SIGNATURES) == names
    assert b"gfx950" in lib.cpd_version()


# ---- every row of _lib.SIGNATURES against its declaration ----
# C scalar type -> (kind, bytes); kind: "i" signed integer, "u" unsigned integer, "f" float. None: no size to compare (void, a struct).
C_TYPES = {"int": ("i", 4), "int32_t": ("i", 4), "long long": ("i", 8), "int64_t": ("i", 8), "size_t": ("u", 8), "float": ("f", 4),
           "double": ("f", 8), "int8_t": ("i", 1), "uint8_t": ("u", 1), "int16_t": ("i", 2), "uint16_t": ("u", 2), "uint32_t": ("u", 4),
           "uint64_t": ("u", 8), "char": ("i", 1), "void": None, "cpd_pack_job": None}
POINTER_BYTES = 8


def header_declarations():
    """include/cpd_hip.h without comments, preprocessor lines and typedefs -> [(name, return type, [parameter, ...])]. A type is
    (pointer depth, base C type): `const float *p` and `const float p[3]` are (1, "float"), `float *const p[3]` is (2, "float"),
    cpd_stream_t is (1, "void")."""
    txt = open(os.path.join(REPO, "include", "cpd_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)
    txt = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*$", " ", txt, flags=re.M)
    txt = re.sub(r'extern\s+"C"\s*\{', " ", txt)
    txt = re.sub(r"\btypedef\s+struct\s*\{.*?\}\s*\w+\s*;", " ", txt, flags=re.S)
    txt = re.sub(r"\btypedef\b[^;{]*;", " ", txt)

    def c_type(text, named):
        depth = text.count("*") + ("[" in text)
        words = re.sub(r"\[[^\]]*\]", " ", text.replace("*", " ")).split()
        words = [w for w in words if w != "const"]
        if named:
            assert len(words) >= 2, "parameter without a name: %r" % text
            words = words[:-1]
        base = " ".join(words)
        if base == "cpd_stream_t":
            depth, base = depth + 1, "void"
        assert base in C_TYPES, "unknown C type %r in %r" % (base, text)
        return depth, base

    out = []
    for stmt in txt.split(";"):
        stmt = " ".join(stmt.split())
        if stmt in ("", "}"):
            continue
        m = re.fullmatch(r"(.*?)\b(cpd_[a-z0-9_]+) ?\(([^()]*)\)", stmt)
        assert m, "not a function declaration: %r" % stmt
        params = [p.strip() for p in m.group(3).split(",")]
        if params in ([""], ["void"]):
            params = []
        out.append((m.group(2), c_type(m.group(1), False), [c_type(p, True) for p in params]))
    return out


def _check_ctype(c_decl, ctype, what):
    depth, base = c_decl
    if depth == 0 and base == "void":
        assert ctype is None, "%s: void needs None, not %r" % (what, ctype)
        return
    assert ctype is not None, "%s: %s needs a ctype" % (what, base)
    is_pointer_ctype = ctype in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(ctype, ctypes._Pointer)
    if depth > 0:
        assert is_pointer_ctype, "%s: a pointer needs c_void_p, c_char_p or POINTER(X), not %r" % (what, ctype)
        if (depth, base) == (1, "char") and what.endswith("return"):
            assert ctype is ctypes.c_char_p, "%s: const char * returns as c_char_p" % what
        if issubclass(ctype, ctypes._Pointer):
            pointee = POINTER_BYTES if depth > 1 else (C_TYPES[base] or (None, None))[1]
            assert pointee is None or ctypes.sizeof(ctype._type_) == pointee, \
                "%s: POINTER(%s) for a pointee of %s bytes" % (what, ctype._type_.__name__, pointee)
        return
    assert not is_pointer_ctype, "%s: the scalar %s needs a scalar ctype, not %r" % (what, base, ctype)
    code = ctype._type_
    kind = "f" if code in "fd" else "i" if code in "bhilq" else "u" if code in "BHILQ" else None
    assert (kind, ctypes.sizeof(ctype)) == C_TYPES[base], "%s: %s is %r, the row has %r" % (what, base, C_TYPES[base], ctype)


def check_signatures(declarations, table):
    """Every declaration has a row whose restype and argtypes match it in arity, pointer-ness, kind and width."""
    assert sorted(table) == sorted(name for name, _, _ in declarations)
    for name, ret, params in declarations:
        restype, argtypes = table[name]
        assert len(argtypes) == len(params), "%s: %d argtypes for %d parameters" % (name, len(argtypes), len(params))
        _check_ctype(ret, restype, "%s return" % name)
        for k, (c_decl, ctype) in enumerate(zip(params, argtypes)):
            _check_ctype(c_decl, ctype, "%s argument %d" % (name, k))


def test_signature_table_matches_every_declaration():
    from cpd_amd import _lib
    declarations = header_declarations()
    names = [name for name, _, _ in declarations]
    assert len(names) >= 178 and len(set(names)) == len(names) and sorted(names) == declared_functions()   # each function once
    check_signatures(declarations, _lib.SIGNATURES)


def _replace_first(argtypes, old, new):
    k = argtypes.index(old)
    return argtypes[:k] + [new] + argtypes[k + 1:]


@pytest.mark.parametrize("name,perturb", [
    ("cpd_index_build", lambda a: a[:-1]),                                                   # an argument dropped
    ("cpd_index_build", lambda a: _replace_first(a, ctypes.c_int, ctypes.c_float)),           # int read as float
    ("cpd_index_build", lambda a: _replace_first(a, ctypes.c_void_p, ctypes.c_int)),          # a pointer read as int
    ("cpd_absmax_rows", lambda a: _replace_first(a, ctypes.c_longlong, ctypes.c_int)),        # long long read at half its width
], ids=["dropped", "int-as-float", "pointer-as-int", "longlong-as-int"])
def test_signature_check_catches_a_wrong_row(name, perturb):
    from cpd_amd import _lib
    table = dict(_lib.SIGNATURES)
    restype, argtypes = table[name]
    table[name] = (restype, perturb(list(argtypes)))
    assert table[name][1] != list(argtypes)
    with pytest.raises(AssertionError, match=name):
        check_signatures(header_declarations(), table)


def test_missing_library_fails_loudly(monkeypatch):
    from cpd_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libcpd_hip.so")
    with pytest.raises(_lib.CpdHipError):
        _lib.lib()


def test_host_geometry_helpers(oracle):
    from cpd_amd import ops
    vs, pcr = [0.1, 0.1, 0.15], [-75.2, -75.2, -2, 75.2, 75.2, 4]
    assert ops.voxel_grid_size(vs, pcr) == oracle.grid_size(vs, pcr) == [40, 1504, 1504]
    assert ops.voxel_grid_size([0.05, 0.05, 0.1], [0, -40, -3, 70.4, 40, 1]) == [40, 1600, 1408]
    for k, s, p in [([3, 3, 3], [2, 2, 2], [1, 1, 1]), ([3, 3, 3], [2, 2, 2], [0, 1, 1]), ([3, 1, 1], [2, 1, 1], [0, 0, 0])]:
        assert ops.conv_out_shape([41, 1504, 1504], k, s, p) == oracle.conv_out_shape([41, 1504, 1504], k, s, p)
    # level shapes of SURVEY section 8: W config
    sh = [41, 1504, 1504]
    for k, s, p in [([3, 3, 3], [2, 2, 2], [1, 1, 1])] * 2 + [([3, 3, 3], [2, 2, 2], [0, 1, 1]), ([3, 1, 1], [2, 1, 1], [0, 0, 0])]:
        sh = ops.conv_out_shape(sh, k, s, p)
    assert sh == [2, 188, 188]


def test_size_queries_and_error_codes():
    from cpd_amd import _lib
    lib = _lib.lib()
    vs, pcr = _lib.farr([0.1, 0.1, 0.15]), _lib.farr([-75.2, -75.2, -2, 75.2, 75.2, 4])
    assert lib.cpd_voxelize_workspace_bytes(160000, 5, 1000000, vs, pcr) > 11 * 2 ** 20
    assert lib.cpd_index_bytes(1, _lib.iarr([41, 1504, 1504]), 100000) > 16 * 2 ** 20
    assert lib.cpd_packed_weight_floats(27, 5, 16) == 27 * 1 * 4 * 16 * 4
    assert lib.cpd_nms_workspace_bytes(500) >= 500 * 8 * 8
    # bad arguments give error codes, never exit()
    assert lib.cpd_gather_conv(None, 0, 0, 0, None, None, None, 0, 0, 0, None, None, None, 0, 0, None, 0, None, 0, 0, None) == -1
    assert lib.cpd_voxelize(None, -1, 5, vs, pcr, 5, 10, 0, 4, None, None, None, None, None, None, 0, None) == -1
    o = (ctypes.c_int32 * 3)()
    assert lib.cpd_conv_out_shape(_lib.iarr([1, 1, 1]), _lib.iarr([3, 3, 3]), _lib.iarr([2, 2, 2]), _lib.iarr([0, 0, 0]), o) == -1


def test_boxes_iou_bev_cpu_entry_point(golden):
    """The extension's one CPU entry point (iou3d_cpu.cpp:232-252) against the reference golden."""
    import torch
    from cpd_amd import ops
    g = golden("iou_bev")
    got = ops.boxes_iou_bev_cpu(torch.from_numpy(g["a"]), torch.from_numpy(g["b"])).numpy()
    np.testing.assert_allclose(got, g["iou_ab"], atol=1e-6, rtol=0)
