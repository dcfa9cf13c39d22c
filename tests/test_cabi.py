"""CPU: the C-ABI library loads and exports every symbol include/rayuela_hip.h declares
(no compute calls -- there is no GPU in the build container)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "rayuela_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(rq_[A-Za-z0-9_]+|linscan_aqd_[a-z_]*query[a-z_]*)\s*\(", src)
    return sorted(set(names))


def test_header_declares_the_reference_symbol():
    assert "linscan_aqd_query" in _declared_symbols()  # deps/src/linscan_aqd.cpp:105-114


def test_library_exports_every_declared_symbol(rq):
    handle = ctypes.CDLL(rq.lib_path())
    for name in _declared_symbols():
        assert hasattr(handle, name), "missing export: " + name


def test_python_binding_covers_the_header(rq):
    from rayuela_jl_amd import _lib
    assert sorted(_lib.SIGNATURES) == _declared_symbols()


def test_version_and_error_channel(rq):
    lib = rq.lib()
    assert b"gfx950" in lib.rq_version()
    assert isinstance(lib.rq_last_error(), bytes)


def test_no_cpu_fallback_without_a_device(rq):
    """On a box without an MI355X the product must fail loudly, not compute on the CPU."""
    import numpy as np
    if rq.lib().rq_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(rq.RayuelaHipError):
        rq.quantize_pq(np.zeros((4, 8), np.float32), [np.zeros((4, 4), np.float32)] * 2)
    with pytest.raises(rq.RayuelaHipError):
        rq.linscan_pq(np.zeros((4, 2), np.uint8), np.zeros((1, 4), np.float32),
                      [np.zeros((256, 2), np.float32)] * 2, 16, 1)


def test_missing_library_is_an_error(monkeypatch, rq):
    from rayuela_jl_amd import _lib
    monkeypatch.setenv("RAYUELA_HIP_LIB", "/nonexistent/librayuela_hip.so")
    monkeypatch.setattr(_lib, "_LIB", None)
    with pytest.raises(_lib.RayuelaHipError):
        _lib.lib()


def test_host_mirror_argument_checks(rq):
    import numpy as np
    # src/Linscan.jl:35: convert(Matrix{UInt8}, B .- 1) throws InexactError for codes outside 1..256
    with pytest.raises(OverflowError):
        rq.linscan_pq(np.array([[0, 1]], dtype=np.int16), np.zeros((1, 4), np.float32),
                      [np.zeros((256, 2), np.float32)] * 2, 16, 1)
    with pytest.raises(ValueError):  # Cint(d/m) InexactError, src/Linscan.jl:23
        rq.linscan_pq(np.zeros((4, 3), np.uint8), np.zeros((1, 4), np.float32),
                      [np.zeros((256, 1), np.float32)] * 3, 24, 1)
    with pytest.raises(TypeError):  # Float64 data never dispatches in the reference (src/PQ.jl:32)
        rq.quantize_pq(np.zeros((4, 8), np.float64), [np.zeros((4, 4), np.float32)] * 2)
    assert [list(p) for p in rq.splitarray(range(1, 11), 4)] == [[1, 2, 3], [4, 5, 6], [7, 8], [9, 10]]


def test_scan_planner_decisions():
    """The planner is pure host code: its work-item decomposition can be checked without a GPU."""
    from rayuela_jl_amd import _lib
    # headline shape: 1250 groups >= 512 resident workgroups, remainder 226 > num_cu/2 -> everything whole
    p = _lib.scan_plan(1_000_000, 10_000, 8, 128, 1000)
    assert p["qg"] == 8 and p["groups"] == 1250 and p["whole"] == 1250 and p["slices"] == 1 and p["grid"] == 512
    assert p["bigk"] == 0 and p["cap"] >= 1000 + 4000
    # 5000 queries: 625 groups = 512 whole + 113 (<= 128) cut in two
    p = _lib.scan_plan(1_000_000, 5_000, 8, 128, 100)
    assert (p["whole"], p["slices"]) == (512, 2) and p["rows_per_slice"] * 2 >= 1_000_000
    # small batch: slices = resident workgroups / groups, never shorter than max(16384, 32 k) rows
    p = _lib.scan_plan(1_000_000, 1_000, 8, 128, 1000)
    assert (p["whole"], p["slices"]) == (0, 4)
    p = _lib.scan_plan(1_000_000, 8, 8, 128, 10)
    assert p["whole"] == 0 and p["slices"] == 41 and p["rows_per_slice"] == 24576   # >= 16384, whole 8192-row blocks
    p = _lib.scan_plan(1_000_000, 8, 8, 128, 10_000)
    assert p["slices"] == 3 and p["bigk"] == 1           # 32 k rows per slice at least; sample-sort finish
    # m = 16 groups 8 queries too, in ONE 1024-thread workgroup per CU (96 KiB of f32 tables + 32 KiB of byte tables);
    # m = 32 groups 4; padded widths plan like the next tiled width
    p = _lib.scan_plan(1_000_000, 10_000, 16, 96, 1000)
    assert p["qg"] == 8 and p["grid"] == 256 and p["whole"] == 1250
    assert _lib.scan_plan(1_000_000, 1_000, 32, 128, 100)["qg"] == 4
    assert _lib.scan_plan(1_000_000, 1_000, 12, 96, 100) == _lib.scan_plan(1_000_000, 1_000, 16, 96, 100)
    # SIFT1B shard: 1.25e8 rows, 1024 queries -> 128 groups over 32 MB row windows (round 2: 4 slices)
    p = _lib.scan_plan(125_000_000, 1024, 8, 128, 100)
    assert (p["groups"], p["slices"], p["xcd"]) == (128, 30, 1)


def test_xcd_window_plan_is_the_default_for_big_bases():
    from rayuela_jl_amd import _lib
    p = _lib.scan_plan(1_000_000_000, 1024, 8, 128, 100)              # BASELINE config 5's workload on one GPU
    assert p["xcd"] == 1 and p["whole"] == 0 and p["slices"] >= 128 and p["rows_per_slice"] * 8 <= 40 << 20, p
    p = _lib.scan_plan(125_000_000, 1024, 8, 128, 100)                # ... and one GPU's shard of it on 8 GPUs
    assert p["xcd"] == 1 and 16 <= p["slices"] <= 64, p
    assert _lib.scan_plan(1_000_000, 10_000, 8, 128, 1000)["xcd"] == 0   # SIFT1M shape: whole-base items


def test_order_plan_host_logic():
    """rq_order_plan (no device): the bank-aware row order spends log2(n / 32) key bits, 3 per leading code byte -- a
    32-value window per byte = one LDS bank column each (csrc/rq_order.hip)."""
    import ctypes as C
    from rayuela_jl_amd import _lib
    L = _lib.lib()

    def plan(n, m):
        out = (C.c_int * 14)()
        assert L.rq_order_plan(n, m, C.cast(out, C.c_void_p), 14) == 0
        return list(out)

    # round 6: where the greedy balance runs (8- and 16-byte rows, two-level sort) the key gives up one table's bits and the rows
    # of a sort bucket are dealt over its lane groups by the uncovered tables: 12 bits + 4 tables at SIFT1M shape
    p = plan(1_000_000, 8)
    assert p[:8] == [3, 3, 3, 3, 0, 0, 0, 0] and p[8] == 12 and p[9] == 32 and p[11] == 8 and p[12] == 4 and p[13] == 16
    from switch_table import switches
    with switches(ORDER_GREEDY=0):
        p = plan(1_000_000, 8)
        assert p[:8] == [3, 3, 3, 3, 3, 0, 0, 0] and p[8] == 15 and p[12] == 0
        assert plan(1_000_000, 16)[:8] == [3, 3, 3, 3, 3, 0, 0, 0]     # m = 16: 5 of 16 tables
    p = plan(1_000_000, 16)
    assert p[:8] == [3, 3, 3, 3, 0, 0, 0, 0] and p[12] == 12 and 8 <= p[13] <= 16
    assert plan(1_000_000, 4)[12] == 0                             # 4-byte rows: the key covers every table already
    p = plan(125_000_000, 8)                       # the per-GPU shard of BASELINE config 5: 22 bits
    assert p[:8] == [3, 3, 3, 3, 3, 3, 3, 1] and p[8] == 22
    assert plan(1_000_000_000, 8)[:9] == [3] * 8 + [24]            # every table conflict-free from 2^29 rows on
    assert plan(500, 8)[8] == 0                                    # tiny base: no ordering
    p = plan(200_000, 5)                                           # padded to 8 bytes; 15/16 of the rows are sorted
    assert p[11] == 8 and p[8] in (12, 13) and p[:4] == [3, 3, 3, 3]
    p = plan(65_536, 2)                                            # narrow rows: both bytes first get a window, then more bits
    assert p[8] == 11 and p[0] + p[1] == 11 and p[2:8] == [0] * 6
    out = (C.c_int * 12)()
    assert L.rq_order_plan(1000, 65, C.cast(out, C.c_void_p), 12) != 0          # m > 64


# ---- typed parity of the three bindings: include/rayuela_hip.h, _lib.SIGNATURES (ctypes), julia/RayuelaHIP.jl (ccall) ----------
# The checkers are pure functions of text / tables, so the negatives below can feed them doctored strings.

_C_SCALARS = {"int": ("int", 4, True), "int64_t": ("int", 8, True), "uint32_t": ("int", 4, False),
              "unsigned": ("int", 4, False), "unsigned int": ("int", 4, False), "uint64_t": ("int", 8, False),
              "size_t": ("int", ctypes.sizeof(ctypes.c_size_t), False), "double": ("float", 8, True)}


def _parse_prototypes(src):
    """{name: (return type, [(type, parameter name), ...])} of every function a C header declares.  Types are normalised:
    no `const`, single blanks, every `*` glued to the type ("uint8_t **")."""
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = re.sub(r"^[ \t]*#[^\n]*(\\\n[^\n]*)*", " ", src, flags=re.M)
    src = re.sub(r'extern\s+"C"\s*\{', " ", src)

    def norm(t):
        t = re.sub(r"\bconst\b", " ", t)
        stars = t.count("*")
        return " ".join(t.replace("*", " ").split()) + (" " + "*" * stars if stars else "")

    protos = {}
    for stmt in src.split(";"):
        stmt = " ".join(stmt.replace("}", " ").split())
        mo = re.match(r"^(.*?)([A-Za-z_]\w*)\s*\((.*)\)$", stmt)
        if not mo or stmt.startswith("typedef"):
            continue
        ret, name, plist = mo.group(1), mo.group(2), mo.group(3).strip()
        params = []
        if plist != "void":
            for p in plist.split(","):
                pm = re.match(r"^(.*?)([A-Za-z_]\w*)$", p.strip())
                assert pm and pm.group(1).strip(), "unnamed parameter in %s: %r" % (name, p)
                params.append((norm(pm.group(1)), pm.group(2)))
        assert name not in protos, "declared twice: " + name
        protos[name] = (norm(ret), params)
    return protos


def _header_prototypes():
    return _parse_prototypes(open(os.path.join(ROOT, "include", "rayuela_hip.h")).read())


def _ctype_class(cls):
    """(kind, size, signed) of a ctypes class, so that aliases (c_int / c_int32, c_uint64 / c_size_t on LP64) compare equal."""
    if cls is None:
        return ("void", 0, False)
    if cls in (ctypes.c_void_p, ctypes.c_char_p):
        return ("pointer", ctypes.sizeof(cls), False)
    if cls in (ctypes.c_double, ctypes.c_float):
        return ("float", ctypes.sizeof(cls), True)
    return ("int", ctypes.sizeof(cls), cls(-1).value < 0)


def _python_mismatches(protos, signatures):
    """Every disagreement between C prototypes and a ctypes (restype, argtypes) table, as readable strings."""
    bad = []

    def want(ctype):
        if ctype == "void":
            return ("void", 0, False)
        if ctype.endswith("*"):
            return ("pointer", ctypes.sizeof(ctypes.c_void_p), False)
        assert ctype in _C_SCALARS, "header type the checker does not know: " + ctype
        return _C_SCALARS[ctype]

    for name, (ret, params) in sorted(protos.items()):
        if name not in signatures:
            bad.append("%s: not bound" % name)
            continue
        res, args = signatures[name]
        if _ctype_class(res) != want(ret):
            bad.append("%s: returns %s, bound as %s" % (name, ret, res))
        if res is ctypes.c_char_p and ret != "char *":
            bad.append("%s: c_char_p for a %s" % (name, ret))
        if len(args) != len(params):
            bad.append("%s: %d parameters, %d bound" % (name, len(params), len(args)))
            continue
        for i, ((ctype, pname), cls) in enumerate(zip(params, args)):
            if _ctype_class(cls) != want(ctype):
                bad.append("%s: parameter %d (%s %s) bound as %s" % (name, i, ctype, pname, cls.__name__))
            elif cls is ctypes.c_char_p and ctype != "char *":
                bad.append("%s: parameter %d (%s %s) bound as c_char_p" % (name, i, ctype, pname))
    return bad


def _split_top(s):
    """Split at the commas outside every bracket and string."""
    out, depth, cur, i = [], 0, [], 0
    while i < len(s):
        c = s[i]
        if c == '"':
            j = s.index('"', i + 1)
            cur.append(s[i:j + 1])
            i = j + 1
            continue
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
        if c == "," and depth == 0:
            out.append("".join(cur).strip())
            cur = []
        else:
            cur.append(c)
        i += 1
    tail = "".join(cur).strip()
    if tail:
        out.append(tail)
    return out


def _parse_ccalls(jl):
    """[(symbol, return type, [argument types], [argument expressions])] of every ccall((:sym, lib), Ret, (T...), a...)."""
    jl = "\n".join(line for line in jl.split("\n") if not line.lstrip().startswith("#"))
    calls = []
    for mo in re.finditer(r"\bccall\(", jl):
        i, depth = mo.end(), 1
        while depth:
            c = jl[i]
            if c == '"':
                i = jl.index('"', i + 1)
            elif c in "([{":
                depth += 1
            elif c in ")]}":
                depth -= 1
            i += 1
        parts = _split_top(jl[mo.end():i - 1])
        assert len(parts) >= 3, "ccall the checker cannot read: " + jl[mo.start():i]
        sym = re.match(r"^\(\s*:(\w+)\s*,\s*\w+\s*\)$", parts[0])
        assert sym and parts[2].startswith("(") and parts[2].endswith(")"), "ccall the checker cannot read: " + jl[mo.start():i]
        calls.append((sym.group(1), parts[1], _split_top(parts[2][1:-1]), parts[3:]))
    return calls


_JL_SCALARS = {"Cint": "int", "Int32": "int", "Int64": "int64_t", "Clonglong": "int64_t", "UInt32": "uint32_t",
               "Cuint": "uint32_t", "UInt64": "uint64_t", "Culonglong": "uint64_t", "Cdouble": "double",
               "Float64": "double", "Csize_t": "size_t"}
_JL_ELEMS = {"Cfloat": "float", "Float32": "float", "Cdouble": "double", "Float64": "double", "UInt8": "uint8_t",
             "Cuchar": "uint8_t", "Int16": "int16_t", "Cshort": "int16_t", "Cuint": "uint32_t", "UInt32": "uint32_t",
             "Cint": "int", "Int32": "int", "Int64": "int64_t", "UInt64": "uint64_t", "Cvoid": "void"}
_C_ALIASES = {"unsigned": "uint32_t", "unsigned int": "uint32_t", "unsigned char": "uint8_t",
              "unsigned long long": "uint64_t"}
_C_ELEMS = {"float", "double", "uint8_t", "int16_t", "uint32_t", "int", "int64_t", "uint64_t"}


def _julia_type_matches(jtype, ctype, is_return=False):
    ctype = _C_ALIASES.get(ctype, ctype)
    if ctype == "void":
        return jtype == "Cvoid"
    if not ctype.endswith("*"):
        return _JL_SCALARS.get(jtype) == ctype
    if ctype == "char *":
        return jtype in ("Cstring", "Ptr{UInt8}", "Ptr{Cchar}")
    pm = re.match(r"^(Ptr|Ref)\{(\w+)\}$", jtype)
    if not pm or (is_return and pm.group(1) != "Ptr"):
        return False
    base = ctype[:-1].strip()
    base = _C_ALIASES.get(base, base)
    if base in _C_ELEMS:
        return _JL_ELEMS.get(pm.group(2)) == base
    return pm.group(2) == "Cvoid"          # void *, an opaque handle struct, a pointer to a pointer


# (symbol, position) pairs excused from the argument-order rule, each with its reason; keep under 5 entries
_ORDER_EXCEPTIONS = {}


def _julia_mismatches(protos, calls, exceptions=_ORDER_EXCEPTIONS):
    """(disagreements between ccalls and C prototypes, number of scalar positions whose argument names the header's parameter)"""
    bad, named = [], 0
    for sym, ret, types, args in calls:
        if sym not in protos:
            bad.append("%s: not declared in the header" % sym)
            continue
        cret, params = protos[sym]
        if not _julia_type_matches(ret, cret, is_return=True):
            bad.append("%s: returns %s, ccall says %s" % (sym, cret, ret))
        if len(types) != len(params) or len(args) != len(params):
            bad.append("%s: %d parameters, %d types and %d arguments in the ccall" % (sym, len(params), len(types), len(args)))
            continue
        scalars = {pname for ctype, pname in params if not ctype.endswith("*")}
        for i, ((ctype, pname), jtype, arg) in enumerate(zip(params, types, args)):
            if not _julia_type_matches(jtype, ctype):
                bad.append("%s: parameter %d (%s %s) passed as %s" % (sym, i, ctype, pname, jtype))
            if ctype.endswith("*"):
                continue
            idents = set(re.findall(r"[A-Za-z_]\w*", re.sub(r'"[^"]*"', " ", arg))) & scalars
            if idents == {pname}:
                named += 1
            elif idents and (sym, i) not in exceptions:
                bad.append("%s: parameter %d is `%s` but the argument `%s` names %s" % (sym, i, pname, arg, sorted(idents)))
    return bad, named


def _julia_source():
    return open(os.path.join(ROOT, "julia", "RayuelaHIP.jl")).read()


def test_prototype_parser_reads_the_whole_header():
    protos = _header_prototypes()
    assert sorted(protos) == _declared_symbols()
    assert protos["rq_dev_rotate_T"] == ("int", [("float *", "RX"), ("float *", "R"), ("float *", "X"), ("int", "d"),
                                                 ("int64_t", "n"), ("void *", "stream")])
    assert protos["rq_version"] == ("char *", []) and protos["rq_host_alloc"] == ("void *", [("size_t", "bytes")])
    assert protos["rq_dev_order_rows"][1][1] == ("uint8_t **", "codes_out")
    assert protos["linscan_aqd_query"][1][6] == ("unsigned int", "NQ") and protos["rq_lsq_release"][0] == "void"


def test_python_binding_types_equal_the_header():
    from rayuela_jl_amd import _lib
    protos = _header_prototypes()
    assert len(protos) >= 88
    assert _python_mismatches(protos, _lib.SIGNATURES) == []


def test_julia_ccalls_equal_the_header():
    protos = _header_prototypes()
    calls = _parse_ccalls(_julia_source())
    assert len(calls) >= 36, len(calls)
    bad, named = _julia_mismatches(protos, calls)
    assert bad == []
    assert named >= 110, named          # the argument-order rule must stay a positive one
    assert len(_ORDER_EXCEPTIONS) < 5


def test_binding_checkers_report_doctored_input():
    """Negatives for the checkers themselves (strings only; no file is touched)."""
    C = ctypes
    protos = _parse_prototypes("int f(float *X, int64_t n, int m, int h, void *stream);\nconst char *g(void);\n"
                               "int s(double *acc, size_t bytes, double rho);")
    good = {"f": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]), "g": (C.c_char_p, []),
            "s": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_double])}
    assert _python_mismatches(protos, good) == []

    def py(**patch):
        return _python_mismatches(protos, dict(good, **patch))

    assert any("parameter 1 (int64_t n)" in b for b in py(f=(C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p])))
    assert any("parameter 2 (int m)" in b for b in py(f=(C.c_int, [C.c_void_p, C.c_int64, C.c_uint32, C.c_int, C.c_void_p])))
    assert any("5 parameters, 4 bound" in b for b in py(f=(C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p])))
    assert any("returns" in b for b in py(f=(None, good["f"][1])))
    assert any("returns" in b for b in py(g=(C.c_int, [])))
    assert any("parameter 2 (double rho)" in b for b in py(s=(C.c_int, [C.c_void_p, C.c_size_t, C.c_int64])))
    assert any("c_char_p" in b for b in py(f=(C.c_int, [C.c_char_p, C.c_int64, C.c_int, C.c_int, C.c_void_p])))
    assert any("not bound" in b for b in _python_mismatches(protos, {"f": good["f"], "g": good["g"]}))

    call = ("_check(ccall((:f, librayuela_hip), Cint, (Ptr{Cfloat}, Int64, Cint, Cint, Ptr{Cvoid}),\n"
            "  X, Int64(n), Cint(m), Cint(h), C_NULL))")
    bad, named = _julia_mismatches(protos, _parse_ccalls(call))
    assert bad == [] and named == 3

    def jl(old, new):
        assert old in call
        return _julia_mismatches(protos, _parse_ccalls(call.replace(old, new)))[0]

    assert any("parameter 2 is `m`" in b for b in jl("Cint(m), Cint(h)", "Cint(h), Cint(m)"))
    assert any("5 parameters, 5 types and 4 arguments" in b for b in jl("Cint(m), Cint(h)", "Cint(m)"))
    assert any("5 parameters, 4 types and 5 arguments" in b for b in jl("Int64, Cint, Cint", "Int64, Cint"))
    assert any("parameter 1 (int64_t n) passed as Cint" in b for b in jl("Int64, Cint", "Cint, Cint"))
    assert any("parameter 0 (float * X) passed as Ptr{Cdouble}" in b for b in jl("Ptr{Cfloat}", "Ptr{Cdouble}"))
    assert any("returns int" in b for b in jl("Cint, (Ptr", "Cvoid, (Ptr"))
    assert any("not declared" in b for b in jl(":f,", ":f2,"))
    dbl = _julia_mismatches(protos, _parse_ccalls("ccall((:s, lib), Cint, (Ptr{Cfloat}, Csize_t, Cdouble), acc, bytes, rho)"))[0]
    assert any("parameter 0 (double * acc) passed as Ptr{Cfloat}" in b for b in dbl)
    # an expression that names no parameter passes; one that names the wrong one among others does not
    assert jl("Cint(h), C_NULL", "Cint(size(C, 2)), C_NULL") == []
    assert any("parameter 3 is `h`" in b for b in jl("Cint(h), C_NULL", "Cint(h * m), C_NULL"))
