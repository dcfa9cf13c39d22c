"""No GPU: the bindings of the additive-quantizer index (rq_index_create_aq[_wide], rq_index_set_codes_aq[_wide],
rq_index_aq_info).  The Python argument checks of AqIndex / AqIndexU16 raise before the library is
called, the header declares the five symbols and _lib.SIGNATURES binds them; tests/test_cabi.py checks their types."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["rq_index_create_aq", "rq_index_create_aq_wide", "rq_index_set_codes_aq", "rq_index_set_codes_aq_wide",
           "rq_index_aq_info"]


@pytest.fixture
def no_library(monkeypatch):
    """Any call into the library fails the test: the checks under test must raise first."""
    from rayuela_jl_amd import _lib

    def boom():
        raise AssertionError("the library was called before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", boom)


def _codebooks(m, h, d, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((h, d)).astype(np.float32) for _ in range(m)]


def _shell(cls, m, h, d, kind):
    """An index object with its shape set and no handle: what set_codes / search check against."""
    ix = object.__new__(cls)
    ix.m, ix.h, ix.d, ix.kind, ix._h, ix.n = m, h, d, kind, None, 0
    return ix


def test_header_declares_the_symbols():
    text = open(os.path.join(ROOT, "include", "rayuela_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"^(rq_index \*|int )%s\(" % name, text, re.M), name
    # host-pointer entries only: none takes a stream (tests/test_gpu_scratch.py pins the set of those that do)
    for name in SYMBOLS:
        proto = re.search(r"^[^\n]*\b%s\(([^;]*)\);" % name, text, re.M | re.S).group(1)
        assert "stream" not in proto, name


def test_signatures_bind_the_symbols():
    import ctypes as C
    from rayuela_jl_amd import _lib
    S = _lib.SIGNATURES
    assert all(name in S for name in SYMBOLS)
    assert S["rq_index_create_aq"][0] is C.c_void_p and len(S["rq_index_create_aq"][1]) == 6
    assert S["rq_index_create_aq_wide"][0] is C.c_void_p and len(S["rq_index_create_aq_wide"][1]) == 7
    assert len(S["rq_index_set_codes_aq"][1]) == 7 and S["rq_index_set_codes_aq"][1][-1] is C.c_uint32
    assert len(S["rq_index_set_codes_aq_wide"][1]) == 8 and S["rq_index_set_codes_aq_wide"][1][-1] is C.c_uint32
    assert S["rq_index_aq_info"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int])
    assert _lib.WS_SLOTS == 20          # no new workspace slot: a handle owns its memory


def test_package_exports_the_classes():
    import rayuela_jl_amd as rq
    assert issubclass(rq.AqIndexU16, rq.AqIndex) and issubclass(rq.AqIndex, rq.Index)
    jl = open(os.path.join(ROOT, "julia", "RayuelaHIP.jl")).read()
    export = [line for line in jl.split("\n") if line.startswith("export") and "HipIndex" in line][0]
    assert "HipAqIndex" in export and "HipAqIndexU16" in export
    for name in SYMBOLS[:4]:
        assert "(:%s, librayuela_hip)" % name in jl, name


@pytest.mark.parametrize("cls,h", [("AqIndex", 256), ("AqIndexU16", 300)])
def test_constructor_checks_come_first(no_library, cls, h):
    import rayuela_jl_amd as rq
    cls = getattr(rq, cls)
    d = 6
    good = _codebooks(4, h, d)
    with pytest.raises(ValueError, match="kind"):
        cls(good, kind="pq")
    with pytest.raises(ValueError, match="1 <= m"):
        cls([])
    with pytest.raises(ValueError, match="1 <= m"):
        cls(_codebooks(cls.M_MAX + 1, 2, 1) if cls.WIDE else [good[0]] * 65)
    with pytest.raises(ValueError):
        cls([c[:, :5] if i == 2 else c for i, c in enumerate(good)])            # one codebook of another dimension
    with pytest.raises(ValueError):
        cls([np.zeros(d, dtype=np.float32)] * 4)                                 # not matrices
    if not cls.WIDE:
        with pytest.raises(ValueError, match="256"):
            cls(_codebooks(4, 100, d))                                           # byte codes: h = 256
    else:
        with pytest.raises(ValueError):
            cls(_codebooks(2, 32768, 1))                                         # past the Int16 limit


@pytest.mark.parametrize("cls,h", [("AqIndex", 256), ("AqIndexU16", 300)])
def test_set_codes_and_search_checks_come_first(no_library, cls, h):
    import rayuela_jl_amd as rq
    cls = getattr(rq, cls)
    m, d, n = 4, 6, 50
    rng = np.random.default_rng(1)
    B = rng.integers(0, min(h, 256), (n, m)).astype(np.uint8 if not cls.WIDE else np.int16)
    nrm = np.ones(n, dtype=np.float32)
    cbn = np.ones(9, dtype=np.float32)
    lsq, cq = _shell(cls, m, h, d, "lsq"), _shell(cls, m, h, d, "cq")
    with pytest.raises(ValueError, match="exactly one"):
        lsq.set_codes(B)
    with pytest.raises(ValueError, match="exactly one"):
        lsq.set_codes(B, dbnorms=nrm, cbnorms=cbn)
    with pytest.raises(ValueError, match="one entry per database row"):
        lsq.set_codes(B, dbnorms=nrm[:-1])
    with pytest.raises(ValueError, match="cbnorms must hold"):
        lsq.set_codes(B, cbnorms=np.zeros(0, dtype=np.float32))
    with pytest.raises(ValueError, match="cbnorms must hold"):
        lsq.set_codes(B, cbnorms=np.zeros(cls.HN_MAX + 1, dtype=np.float32))
    with pytest.raises(ValueError, match="no norms"):
        cq.set_codes(B, dbnorms=nrm)
    with pytest.raises(ValueError, match="no norms"):
        cq.set_codes(B, cbnorms=cbn)
    with pytest.raises(ValueError, match="codes must be"):
        cq.set_codes(B[:, :3])
    with pytest.raises(TypeError):
        cq.set_codes(B.astype(np.float32))
    with pytest.raises(OverflowError):
        cq.set_codes(np.zeros((n, m), dtype=np.int32))                           # wider integers are ONE-based: 0 is no code
    if cls.WIDE:
        with pytest.raises(OverflowError):
            cq.set_codes(np.full((n, m), h, dtype=np.int16))                     # zero-based: h is out of range
    with pytest.raises(ValueError, match="d="):
        lsq.search(np.zeros((3, d + 1), dtype=np.float32), 5)
    with pytest.raises(ValueError, match="R must be"):
        lsq.search(np.zeros((3, d), dtype=np.float32), 5, R=np.eye(d + 1, dtype=np.float32))
    with pytest.raises(NotImplementedError):
        lsq.set_codes_synth(10, 1)
    assert lsq.n == 0 and cq.n == 0
