"""CPU: rq_train_sr_wide (LSQ++ over 16-bit codes) refuses bad arguments with the status its contract
names, before a device is needed and without writing an output byte; the Python mirrors refuse the same cases before the
library is loaded and route by h."""
import numpy as np
import pytest

RQ_EINVAL, RQ_EUNSUPPORTED = -1, -2
SR_C, SR_D = 0, 1


def test_status_codes_are_the_headers(rq):
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rayuela_hip.h")).read()
    for name, val in (("RQ_EINVAL", RQ_EINVAL), ("RQ_EUNSUPPORTED", RQ_EUNSUPPORTED), ("RQ_SR_RECOMPUTE", 1)):
        mo = re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % name, src)
        assert mo and int(mo.group(1)) == val, name


def test_c_abi_argument_checks(rq):
    L = rq.lib()
    n, d, m, h = 4, 8, 2, 300
    X = np.zeros((n, d), np.float32)
    R = np.eye(d, dtype=np.float32)
    B = np.full((n, m), h - 1, np.int16)
    C = np.full((m, h, d), -5.0, np.float32)
    obj = np.full(3, -5.0)
    codes_io = B.copy()
    p = lambda a: None if a is None else a.ctypes.data             # noqa: E731

    def train(**kw):
        a = dict(n=n, d=d, m=m, h=h, X=X, R=R, codes=codes_io, out=C, obj=obj, niter=2, ils=1, icm=1, npert=1, method=SR_D,
                 schedule=1, p=0.5, clean=1, ns=1, base=0, flags=0)
        a.update(kw)
        return L.rq_train_sr_wide(p(a["out"]), p(a["codes"]), p(a["obj"]), p(a["X"]), p(a["R"]), a["n"], a["d"], a["m"], a["h"],
                                  a["niter"], a["ils"], a["icm"], a["npert"], 1, a["method"], a["schedule"], a["p"], a["clean"],
                                  7, a["ns"], a["base"], a["flags"])

    one = np.full((1, m), h - 1, np.int16)
    cases = [(dict(h=32768), b"h=32768"), (dict(h=1), b"h=1"), (dict(m=17), b"m=17"), (dict(m=0), b"m=0"), (dict(d=0), b"d=0"),
             (dict(n=-1), b"n=-1"), (dict(n=1 << 32), b"n=4294967296"),
             (dict(base=2), b"code_base"), (dict(base=-1), b"code_base"),
             (dict(flags=2), b"flags"), (dict(flags=3), b"flags"), (dict(flags=-1), b"flags"),
             (dict(method=2), b"method 2"), (dict(method=-1), b"method -1"),
             (dict(niter=0), b"niter=0"), (dict(niter=-1), b"niter=-1"),
             (dict(method=SR_C, n=1, codes=one), b"SR_C needs n >= 2"), (dict(method=SR_C, n=0), b"SR_C needs n >= 2"),
             (dict(schedule=4), b"schedule=4"), (dict(schedule=0), b"schedule=0"),
             (dict(p=-1.0), b"p="), (dict(p=float("nan")), b"p="), (dict(p=float("inf")), b"p="),
             (dict(codes=B + 1), b"code 300 at [0][0] is outside 0..299"), (dict(codes=B - h), b"code -1 at [0][0]"),
             (dict(codes=B - (h - 1), base=1), b"code 0 at [0][0] is outside 1..300"),
             (dict(codes=B + 2, base=1), b"code 301 at [0][0] is outside 1..300"),
             (dict(out=None), b"null"), (dict(codes=None), b"null"), (dict(obj=None), b"null"), (dict(X=None), b"null"),
             (dict(npert=3), b"npert=3"), (dict(npert=-1), b"npert=-1"), (dict(ils=-1), b"negative"), (dict(icm=-1), b"negative"),
             (dict(ns=0), b"nsplits"), (dict(ils=1 << 30), b"overflows")]
    for kw, word in cases:
        assert train(**kw) == RQ_EINVAL, kw
        assert word in L.rq_last_error(), (kw, L.rq_last_error())
    # m * h = 16640 passes the encoder's table rule and is past the update's limit
    assert train(m=13, h=1280, codes=np.zeros((n, 13), np.int16)) == RQ_EUNSUPPORTED
    assert b"exceeds 16384" in L.rq_last_error()
    # shapes rq_icm_wide_plan refuses (the pair tables past the encoder's scratch)
    for mm, hh in ((16, 2048), (2, 16384)):
        none = np.zeros(1, np.int64)
        assert L.rq_icm_wide_plan(n, d, mm, hh, 1, none.ctypes.data, 0) == RQ_EUNSUPPORTED
        assert train(m=mm, h=hh, codes=np.zeros((n, mm), np.int16)) == RQ_EUNSUPPORTED, (mm, hh)
    # R is optional: a null R is no refusal, and neither is the largest m * h.  Without a device such a call passes every check
    # and only then fails to find one.
    if L.rq_device_count() <= 0:
        for kw in (dict(R=None), dict(m=16, h=1024, codes=np.zeros((n, 16), np.int16), out=np.zeros((16, 1024, d), np.float32)),
                   dict(method=SR_C, flags=1), dict(base=1, codes=B + 1)):
            assert train(**kw) not in (0, RQ_EINVAL, RQ_EUNSUPPORTED), kw
    # no output byte was written by any refusal
    assert (C == -5.0).all() and (obj == -5.0).all() and np.array_equal(codes_io, B)


def test_last_sr_stats_refuses_a_null_pointer(rq):
    L = rq.lib()
    assert L.rq_last_sr_stats(None, 3) == RQ_EINVAL
    out = np.full(4, -7, np.int64)
    assert L.rq_last_sr_stats(out.ctypes.data, 0) == 0 and (out == -7).all()
    assert L.rq_last_sr_stats(out.ctypes.data, 8) == 0 and out[3] == -7 and (out[:3] >= 0).all()     # three entries at the most


def _args(n=6, d=4, m=2, h=300):
    rng = np.random.default_rng(2)
    B = rng.integers(1, h + 1, size=(n, m)).astype(np.int16)
    B[0, 0], B[0, 1] = h, 1                               # both ends of the one-based range
    return rng.standard_normal((n, d)).astype(np.float32), B


def test_python_argument_checks_run_before_the_library(rq, monkeypatch):
    from rayuela_jl_amd import _lib
    from rayuela_jl_amd.SR import train_sr_u16
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    X, B = _args()
    big = np.ones((6, 16), np.int16)
    cuda = lambda h=300, B=B, m=2, R=None, niter=1, method="SR_D", schedule=1, p=0.5, nsplits=1, npert=1, X=X: (   # noqa: E731
        rq.train_sr_cuda(X, m, h, R, B, None, niter, 1, 1, True, npert, method, schedule, p, nsplits))
    u16 = lambda codes=B - 1, m=2, h=300, niter=1, method="SR_D", schedule=1, **kw: (                                # noqa: E731
        train_sr_u16(X, codes, m, h, None, niter, 1, 1, True, 1, method, schedule, **kw))
    bad = [
        lambda: cuda(h=32768),                                                   # h past the Int16 limit
        lambda: cuda(m=17, B=np.ones((6, 17), np.int16)),
        lambda: cuda(m=13, h=1280, B=np.ones((6, 13), np.int16)),                # m * h = 16640
        lambda: cuda(m=16, h=2048, B=big),                                       # the encoder's tables do not fit
        lambda: cuda(method="SR_E"),
        lambda: cuda(method=2),
        lambda: cuda(niter=0),
        lambda: cuda(method="SR_C", X=X[:1], B=B[:1]),                           # SR_C with n = 1
        lambda: cuda(schedule=4),
        lambda: cuda(p=-1.0),
        lambda: cuda(B=B + 1),                                                   # a code equal to code_base + h
        lambda: cuda(B=B - 1),                                                   # a code below code_base
        lambda: cuda(nsplits=0),
        lambda: cuda(npert=3),
        lambda: cuda(R=np.eye(3, dtype=np.float32)),
        lambda: rq.train_sr(X, 2, 300, None, B.copy(), None, 1, 1, 1, True, 1, "SR_D", 0.5),                 # cpp=True: h = 256
        lambda: rq.train_sr(X, 2, 300, None, B + 1, None, 1, 1, 1, True, 1, "SR_D", 0.5, cpp=False),
        lambda: rq.train_sr(X, 2, 300, None, B.copy(), None, 0, 1, 1, True, 1, "SR_C", 0.5, cpp=False),
        lambda: u16(codes=B),                                                    # one-based codes: 300 >= h
        lambda: u16(codes=B - 2),                                                # a code below zero
        lambda: u16(m=3),
        lambda: u16(h=32768),
        lambda: u16(niter=0),
        lambda: u16(schedule=4),
        lambda: u16(method="SR_C", p=float("nan")),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail("case %d raised nothing" % i)
    with pytest.raises(TypeError):
        cuda(B=B.astype(np.int32))
    # h > 256 passes every mirror's checks and reaches the (patched) library
    for f in (cuda, lambda: cuda(method="SR_C", schedule=3), lambda: cuda(m=16, h=1024, B=big), u16,
              lambda: u16(recompute=True), lambda: u16(method="SR_C", clean_update=False),
              lambda: rq.train_sr(X, 2, 300, None, B.copy(), None, 1, 1, 1, True, 1, "SR_D", 0.5, cpp=False)):
        with pytest.raises(AssertionError, match="library touched"):
            f()


def test_mirrors_route_by_h(rq, monkeypatch):
    """h <= 256 keeps the byte loop, h > 256 takes the one over 16-bit codes; both see zero-based codes of their own width, and
    the caller gets one-based Int16 codes back (train_sr also in B, train_sr_cuda not)."""
    from rayuela_jl_amd import SR
    seen = []

    def fake(name, dtype):
        def fn(X, codes0, m, h, R, niter, ilsiter, icmiter, randord, npert, method, schedule=1, p=0.5, clean_update=True, seed=0,
               nsplits=1, **kw):
            assert codes0.dtype == dtype and codes0.min() == 0 and codes0.max() == h - 1 and not kw
            seen.append((name, bool(clean_update), schedule))
            return np.zeros((m, h, X.shape[1]), np.float32), np.array(codes0[::-1], dtype=dtype), np.zeros(niter + 1)
        return fn
    monkeypatch.setattr(SR, "train_sr_u8", fake("t8", np.uint8))
    monkeypatch.setattr(SR, "train_sr_u16", fake("t16", np.int16))
    for h, tr in ((256, "t8"), (257, "t16")):
        X, B = _args(h=h)
        keep = B.copy()
        Cn, Bn, obj = rq.train_sr(X, 2, h, None, B, None, 2, 1, 1, True, 1, "SR_C", 0.5, cpp=False)
        assert Bn.dtype == np.int16 and np.array_equal(Bn, keep[::-1]) and np.array_equal(B, Bn)
        assert obj.dtype == np.float32 and obj.shape == (3,) and len(Cn) == 2 and Cn[0].shape == (h, 4)
        B = keep.copy()
        Cn, Bn, obj = rq.train_sr_cuda(X, 2, h, None, B, None, 2, 1, 1, True, 1, "SR_D", 3)
        assert Bn.dtype == np.int16 and np.array_equal(Bn, keep[::-1]) and np.array_equal(B, keep)
        assert seen == [(tr, False, 1), (tr, True, 3)]
        del seen[:]


def test_last_sr_stats_mirror(rq):
    from rayuela_jl_amd.SR import last_sr_stats
    s = last_sr_stats()
    assert sorted(s) == ["full", "reused", "skipped"] and all(isinstance(v, int) and v >= 0 for v in s.values())
