"""CPU: the chain quantization restatement over int16 codes (tests/chain_wide_oracle.py) against tests/chain_oracle.py where both
run, the known answers of rq_chain_wide_plan, the argument checks of the three rq_*_chain*_wide entries (no device is needed for
any of them) and the Python mirrors' checks and routing."""
import ctypes

import numpy as np
import pytest

import chain_oracle as co
import chain_wide_oracle as cw

GIB2 = 2 << 30


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- the helper against the byte restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,h,d,n", [(3, 40, 9, 50), (5, 65, 30, 33)])
def test_helper_equals_the_byte_restatement(oracle, m, h, d, n):
    rng = np.random.default_rng(m + h)
    X = rng.standard_normal((n, d)).astype(np.float32)
    C = (rng.standard_normal((m, h, d)) * 0.5).astype(np.float32)
    U, T = co.tables(oracle, X, C)
    Uw, Tw = cw.tables(oracle, X, C)
    assert _same_bits(U, Uw) and _same_bits(T, Tw)
    want = co.viterbi(oracle, X, C)
    for blk in (1, 7, 64):
        got = cw.viterbi(oracle, X, C, block=blk)
        assert got.dtype == np.int16 and np.array_equal(got, want)
    codes = rng.integers(0, h, size=(600, m)).astype(np.uint8)
    Xu = rng.standard_normal((600, d)).astype(np.float32)
    Cb, Cb64 = co.chain_update(Xu, codes, h)
    Cn, Cn64 = cw.chain_update(Xu, codes.astype(np.int16), h)
    assert _same_bits(Cb, Cn) and _same_bits(Cb64, Cn64)


def test_helper_train_equals_the_byte_restatement(oracle):
    rng = np.random.default_rng(4)
    n, d, m, h = 300, 8, 3, 16
    X = rng.standard_normal((n, d)).astype(np.float32)
    B = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    R = np.eye(d, dtype=np.float32)
    a = co.train(oracle, X, B, R, h, 1)
    b = cw.train(oracle, X, B.astype(np.int16), R, h, 1)
    assert _same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and _same_bits(a[2], b[2]) and _same_bits(a[3], b[3])


# ---- rq_chain_wide_plan -----------------------------------------------------------------------------------------------------------
def _plan(L, n, d, m, h, nsplits=1, cap=7, fill=-7):
    out = (ctypes.c_int64 * 8)(*([fill] * 8))
    rc = L.rq_chain_wide_plan(n, d, m, h, nsplits, ctypes.cast(out, ctypes.c_void_p), cap)
    return rc, list(out)


def _expect(n, m, h, nsplits):
    HS = 64 * ((h + 63) // 64)
    T = 2 * (m - 1) * h * HS * 4 + m * h * 4
    row = m * HS * 4
    chunk = 0 if n == 0 else max(1, min(-(-n // nsplits), (GIB2 - T) // row))
    chunks = 0 if n == 0 else -(-n // chunk)
    return [HS, T, row, chunk, chunks, (2 * h) ** 2 * 8]


def test_plan_known_answers(rq):
    from rayuela_jl_amd import _lib
    L = _lib.lib()
    # (m, h) = (8, 4096): T = 2 * 7 * 4096 * 4096 * 4 + 8 * 4096 * 4, one row of unaries 8 * 4096 * 4
    rc, out = _plan(L, 100000, 128, 8, 4096)
    assert rc == 0 and out[:3] == [4096, 939655168, 131072]
    assert out[3] == (GIB2 - 939655168) // 131072 == 9215 and out[4] == 11 and out[5] == 8192 * 8192 * 8 and out[6] == 1
    rc, out = _plan(L, 100000, 128, 16, 2048, nsplits=3)
    assert rc == 0 and out[:3] == [2048, 2 * 15 * 2048 * 2048 * 4 + 16 * 2048 * 4, 16 * 2048 * 4]
    assert out[3] == min(33334, (GIB2 - out[1]) // out[2]) and out[4] == -(-100000 // out[3]) and out[6] == 1
    rc, out = _plan(L, 5000, 64, 4, 8192)
    assert rc == 0 and out[:3] == [8192, 2 * 3 * 8192 * 8192 * 4 + 4 * 8192 * 4, 4 * 8192 * 4]
    assert out[3] == (GIB2 - out[1]) // out[2] == 4095 and out[4] == 2 and out[5] == 2 ** 31 and out[6] == 1
    # every shape against the rule as the header states it
    for n, d, m, h, ns in [(1000, 16, 3, 300, 1), (1000, 16, 3, 300, 7), (77, 8, 1, 257, 2), (10, 20, 16, 2, 1), (9, 4, 2, 10000, 1),
                            (3, 4, 1, 32767, 1)]:
        rc, out = _plan(L, n, d, m, h, ns)
        assert rc == 0 and out[:6] == _expect(n, m, h, ns), (n, d, m, h, ns, out)
    # HS: a partial group of 64 rounds up, a full one does not
    assert _plan(L, 1, 8, 2, 300)[1][0] == 320 and _plan(L, 1, 8, 2, 320)[1][0] == 320 and _plan(L, 1, 8, 2, 257)[1][0] == 320
    # the tables of (2, 16384) alone are 2 GiB
    rc, out = _plan(L, 100, 8, 2, 16384)
    assert rc == -2 and b"16384" in L.rq_last_error() and out == [-7] * 8
    # the update / training flag: 2 h <= 16384, m >= 2, m - 1 <= d <= 1024
    assert _plan(L, 100, 8, 2, 8192)[1][6] == 1
    rc, out = _plan(L, 100, 8, 2, 8193)
    assert rc == 0 and out[6] == 0
    assert _plan(L, 100, 8, 1, 300)[1][6] == 0 and _plan(L, 100, 2, 4, 300)[1][6] == 0 and _plan(L, 100, 1025, 4, 300)[1][6] == 0
    assert _plan(L, 100, 1024, 4, 300)[1][6] == 1
    # n = 0: no rows per chunk and no chunks
    rc, out = _plan(L, 0, 8, 4, 300)
    assert rc == 0 and out[3] == 0 and out[4] == 0 and out[0] == 320
    # cap is honoured
    rc, out = _plan(L, 100, 8, 4, 300, cap=3)
    assert rc == 0 and out[:3] == _expect(100, 4, 300, 1)[:3] and out[3:] == [-7] * 5
    rc, out = _plan(L, 100, 8, 4, 300, cap=0)
    assert rc == 0 and out == [-7] * 8
    rc, out = _plan(L, 100, 8, 4, 300, cap=20)
    assert rc == 0 and out[7] == -7
    # bad shapes are RQ_EINVAL
    for args, word in [((10, 8, 0, 300), b"m=0"), ((10, 8, 17, 300), b"m=17"), ((10, 8, 2, 1), b"h=1"), ((10, 8, 2, 32768), b"h=32768"),
                       ((10, 0, 2, 300), b"d=0"), ((-1, 8, 2, 300), b"negative"), ((10, 8, 2, 300, 0), b"nsplits")]:
        rc, out = _plan(L, *args)
        assert rc == -1 and word in L.rq_last_error() and out == [-7] * 8, (args, L.rq_last_error())
    assert L.rq_chain_wide_plan(10, 8, 2, 300, 1, None, 7) == -1
    assert L.rq_chain_wide_plan(10, 8, 2, 300, 1, ctypes.cast((ctypes.c_int64 * 8)(), ctypes.c_void_p), -1) == -1


# ---- the C ABI's argument checks ----------------------------------------------------------------------------------------------------
def test_c_abi_argument_checks_touch_no_output(rq):
    """Every refusal of the three wide entries comes through rq_last_error before any device is needed, and leaves the outputs as
    they were."""
    from rayuela_jl_amd import _lib
    L = _lib.lib()
    n, d, m, h = 4, 8, 2, 300
    X = np.zeros((n, d), np.float32)
    Cin = np.zeros((17, 4, d), np.float32)                        # enough for every refused (m, h) the encoder could look at
    R = np.eye(d, dtype=np.float32)
    p = lambda a: None if a is None else a.ctypes.data     # noqa: E731
    state = {}

    def fresh():
        state["codes"] = np.full((n, m), 5, np.int16)
        state["C"] = np.full((m, h, d), 7, np.float32)
        state["R"] = R.copy()
        state["obj"] = np.full(3, 9.0)

    def untouched():
        return ((state["codes"] == 5).all() and (state["C"] == 7).all() and np.array_equal(state["R"], R)
                and (state["obj"] == 9).all())

    def enc(m=m, h=h, d=d, n=n, ns=1, base=0, codes=True, Xp=X, Cp=Cin):
        return L.rq_quantize_chainq_wide(p(state["codes"]) if codes else None, p(Xp), p(Cp), n, d, m, h, ns, base)

    def upd(m=m, h=h, d=d, n=n, rho=1e-4, base=0, codes=None, Cout=True, Xp=X):
        c = state["codes"] if codes is None else codes
        return L.rq_update_codebooks_chain_wide(p(state["C"]) if Cout else None, p(Xp), p(c), n, d, m, h, rho, base)

    def trn(m=m, h=h, d=d, n=n, niter=2, base=0, codes=None, Rp=True, objp=True, Xp=X):
        c = state["codes"] if codes is None else codes
        return L.rq_train_chainq_wide(p(state["C"]), p(c), p(state["R"]) if Rp else None, p(state["obj"]) if objp else None, p(Xp),
                                      n, d, m, h, niter, base)
    lo0, hi0 = np.full((n, m), -1, np.int16), np.full((n, m), h, np.int16)       # code_base - 1 and code_base + h at base 0
    lo1, hi1 = np.zeros((n, m), np.int16), np.full((n, m), h + 1, np.int16)      # the same at base 1
    cases = [
        (lambda: enc(m=0), -1, b"m=0"), (lambda: enc(m=17), -1, b"m=17"), (lambda: enc(h=1), -1, b"h=1"),
        (lambda: enc(h=32768), -1, b"h=32768"), (lambda: enc(base=2), -1, b"code_base"), (lambda: enc(base=-1), -1, b"code_base"),
        (lambda: enc(d=0), -1, b"d=0"), (lambda: enc(n=-1), -1, b"negative"), (lambda: enc(ns=0), -1, b"nsplits"),
        (lambda: enc(codes=False), -1, b"null"), (lambda: enc(Xp=None), -1, b"null"), (lambda: enc(Cp=None), -1, b"null"),
        (lambda: enc(h=16384), -2, b"16384"),
        (lambda: upd(m=0), -1, b"m=0"), (lambda: upd(m=1), -1, b"m=1"), (lambda: upd(m=17), -1, b"m=17"), (lambda: upd(h=1), -1, b"h=1"),
        (lambda: upd(h=32768), -1, b"h=32768"), (lambda: upd(base=2), -1, b"code_base"), (lambda: upd(rho=0.0), -1, b"rho"),
        (lambda: upd(rho=float("inf")), -1, b"rho"), (lambda: upd(m=4, d=2), -1, b"m - 1"), (lambda: upd(Cout=False), -1, b"null"),
        (lambda: upd(Xp=None), -1, b"null"), (lambda: upd(codes=lo0), -1, b"outside 0..299"),
        (lambda: upd(codes=hi0), -1, b"outside 0..299"), (lambda: upd(codes=lo1, base=1), -1, b"outside 1..300"),
        (lambda: upd(codes=hi1, base=1), -1, b"outside 1..300"), (lambda: upd(h=8193), -2, b"16386"),
        (lambda: trn(m=0), -1, b"m=0"), (lambda: trn(m=1), -1, b"m=1"), (lambda: trn(m=17), -1, b"m=17"), (lambda: trn(h=1), -1, b"h=1"),
        (lambda: trn(h=32768), -1, b"h=32768"), (lambda: trn(base=2), -1, b"code_base"), (lambda: trn(niter=-1), -1, b"niter"),
        (lambda: trn(n=0), -1, b"n=0"), (lambda: trn(m=4, d=2), -1, b"m - 1"), (lambda: trn(Rp=False), -1, b"null"),
        (lambda: trn(objp=False), -1, b"null"), (lambda: trn(Xp=None), -1, b"null"), (lambda: trn(codes=lo0), -1, b"outside 0..299"),
        (lambda: trn(codes=hi0), -1, b"outside 0..299"), (lambda: trn(codes=lo1, base=1), -1, b"outside 1..300"),
        (lambda: trn(codes=hi1, base=1), -1, b"outside 1..300"), (lambda: trn(d=1025), -2, b"1024"),
        (lambda: trn(h=8193), -2, b"16386"), (lambda: trn(h=16384), -2, b"16384"),
    ]
    for k, (call, rc, word) in enumerate(cases):
        fresh()
        assert call() == rc, (k, L.rq_last_error())
        assert word in L.rq_last_error(), (k, L.rq_last_error())
        assert untouched(), k
    # n = 0 encodes nothing and needs no device
    fresh()
    assert enc(n=0) == 0 and untouched()


# ---- the Python mirrors -------------------------------------------------------------------------------------------------------------
def _args(n=10, d=8, m=4, h=257):
    rng = np.random.default_rng(2)
    B = rng.integers(1, h + 1, size=(n, m)).astype(np.int16)
    B[0, 0], B[0, 1] = h, 1                               # both ends of the one-based range
    return (rng.standard_normal((n, d)).astype(np.float32), B, [rng.standard_normal((h, d)).astype(np.float32) for _ in range(m)])


def test_python_argument_checks_run_before_the_library(rq, monkeypatch):
    from rayuela_jl_amd import _lib
    from rayuela_jl_amd.ChainQ import quantize_chainq_u16, train_chainq_u16
    from rayuela_jl_amd.codebook_update import update_codebooks_chain_bin_u16
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    X, B, C = _args()
    R = np.eye(8, dtype=np.float32)
    X17, B17, C17 = _args(m=17, d=20)
    Xh, Bh, Ch = _args(h=1)
    z = lambda h, m=2: [np.zeros((h, 8), np.float32)] * m      # noqa: E731
    bad = [
        lambda: rq.quantize_chainq(X, C),                                          # h = 257 without wide: the byte contract stays
        lambda: rq.update_codebooks_chain_bin(X, B, 257),
        lambda: rq.quantize_chainq(X[:, :4], C, wide=True),                        # d mismatch
        lambda: rq.quantize_chainq(X, [], wide=True),                              # m = 0
        lambda: rq.quantize_chainq(X17, C17, wide=True),                           # m = 17
        lambda: rq.quantize_chainq(Xh, Ch, wide=True),                             # h = 1
        lambda: rq.quantize_chainq(X, z(32768), wide=True),                        # h past the Int16 limit
        lambda: rq.quantize_chainq(X, z(16384), wide=True),                        # the tables alone are 2 GiB
        lambda: quantize_chainq_u16(X, C, nsplits=0),
        lambda: rq.update_codebooks_chain_bin(X, B[:, :1], 257, wide=True),        # update with m = 1
        lambda: rq.update_codebooks_chain_bin(X, B17, 257, wide=True),             # m = 17
        lambda: rq.update_codebooks_chain_bin(X, B, 256, wide=True),               # a code past h
        lambda: rq.update_codebooks_chain_bin(X, B - 1, 257, wide=True),           # zero-based codes
        lambda: rq.update_codebooks_chain_bin(X, B, 8193, wide=True),              # 2 h > 16384
        lambda: rq.update_codebooks_chain_bin(X, B, 32768, wide=True),
        lambda: rq.update_codebooks_chain_bin(X, B[:5], 257, wide=True),           # wrong shape
        lambda: rq.update_codebooks_chain_bin(X, B, 257, rho=0.0, wide=True),
        lambda: rq.update_codebooks_chain_bin(X[:, :2], B, 257, wide=True),        # d < m - 1
        lambda: update_codebooks_chain_bin_u16(X, B, 257),                         # one-based codes: 257 >= h
        lambda: rq.train_chainq(X, 4, 256, R, B, None, 1),                         # a code past h
        lambda: rq.train_chainq(X, 4, 257, R[:4], B, None, 1),                     # R shape
        lambda: rq.train_chainq(X, 4, 257, R, B, None, -1),                        # niter
        lambda: rq.train_chainq(X, 3, 257, R, B, None, 1),                         # m against the codes
        lambda: rq.train_chainq(X, 4, 8193, R, B, None, 1),                        # 2 h > 16384
        lambda: train_chainq_u16(X, B, 4, 257, R, 1),                              # one-based codes
        lambda: train_chainq_u16(np.zeros((10, 1025), np.float32), B - 1, 4, 257, np.eye(1025, dtype=np.float32), 1),
    ]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail("case %d raised nothing" % k)
    with pytest.raises(TypeError):
        rq.quantize_chainq(X.astype(np.float64), C, wide=True)
    with pytest.raises(TypeError):
        rq.train_chainq(X, 4, 257, R, B.astype(np.int32), None, 1)
    with pytest.raises(TypeError):
        rq.quantize_chainq(X, C, False, False, True)                               # wide is keyword only
    # good arguments pass the checks and reach the (patched) library; wide=True also takes h <= 256
    Xs, Bs, Cs = _args(h=100)
    for f in (lambda: rq.quantize_chainq(X, C, wide=True), lambda: rq.quantize_chainq(X, C, True, True, wide=True),
              lambda: quantize_chainq_u16(X, C, nsplits=3), lambda: rq.quantize_chainq(Xs, Cs, wide=True),
              lambda: rq.quantize_chainq(X, z(8192, 4), wide=True),
              lambda: rq.update_codebooks_chain_bin(X, B, 257, wide=True), lambda: update_codebooks_chain_bin_u16(X, B - 1, 257),
              lambda: rq.update_codebooks_chain_bin(Xs, Bs, 100, wide=True), lambda: rq.update_codebooks_chain_bin(X, B, 8192, wide=True),
              lambda: rq.train_chainq(X, 4, 257, R, B, None, 1), lambda: train_chainq_u16(X, B - 1, 4, 257, R, 0),
              lambda: train_chainq_u16(Xs, Bs - 1, 4, 100, R, 1)):
        with pytest.raises(AssertionError, match="library touched"):
            f()


def test_mirrors_route_by_h(rq, monkeypatch):
    """train_chainq: h <= 256 keeps the byte loop, h > 256 takes the loop over 16-bit codes; both see zero-based codes of their own
    width and the caller gets one-based Int16 codes back, its own array left alone.  quantize_chainq and update_codebooks_chain_bin
    route by `wide` alone."""
    from rayuela_jl_amd import ChainQ, codebook_update
    seen = []

    def fake_train(name, dtype, out):
        def fn(X, codes0, m, h, R, niter):
            assert codes0.dtype == dtype and codes0.min() == 0 and codes0.max() == h - 1
            seen.append(name)
            return (np.zeros((m, h, X.shape[1]), np.float32), np.array(codes0[::-1]).astype(out), np.asarray(R), np.zeros(niter + 1))
        return fn
    monkeypatch.setattr(ChainQ, "train_chainq_u8", fake_train("t8", np.int16, np.uint8))
    monkeypatch.setattr(ChainQ, "train_chainq_u16", fake_train("t16", np.int16, np.uint16))
    for h, tr in ((256, "t8"), (257, "t16"), (8192, "t16")):
        X, B, _ = _args(h=h)
        keep = B.copy()
        Cn, Bn, Rn, obj = rq.train_chainq(X, 4, h, np.eye(8, dtype=np.float32), B, None, 2)
        assert seen == [tr] and Bn.dtype == np.int16 and np.array_equal(Bn, keep[::-1]) and np.array_equal(B, keep)
        assert len(Cn) == 4 and Cn[0].shape == (h, 8) and obj.dtype == np.float32 and obj.shape == (3,)
        del seen[:]

    def fake_enc(name, dtype):
        def fn(X, C, nsplits=1):
            seen.append(name)
            return np.full((X.shape[0], len(C)), len(C[0]) - 1, dtype)
        return fn
    monkeypatch.setattr(ChainQ, "quantize_chainq_u8", fake_enc("q8", np.uint8))
    monkeypatch.setattr(ChainQ, "quantize_chainq_u16", fake_enc("q16", np.uint16))
    X, B, C = _args(h=300)
    Bq, _ = rq.quantize_chainq(X, C, wide=True)
    assert seen == ["q16"] and Bq.dtype == np.int16 and (Bq == 300).all()
    del seen[:]
    Xs, Bs, Cs = _args(h=256)
    assert (rq.quantize_chainq(Xs, Cs)[0] == 256).all() and (rq.quantize_chainq(Xs, Cs, wide=True)[0] == 256).all()
    assert seen == ["q8", "q16"]
    del seen[:]

    def fake_upd(name, dtype):
        def fn(X, codes, h, rho=1e-4):
            assert codes.dtype == dtype and codes.min() == 0 and codes.max() == h - 1
            seen.append(name)
            return np.zeros((codes.shape[1], h, X.shape[1]), np.float32)
        return fn
    monkeypatch.setattr(codebook_update, "update_codebooks_chain_u8", fake_upd("u8", np.uint8))
    monkeypatch.setattr(codebook_update, "update_codebooks_chain_bin_u16", fake_upd("u16", np.int16))
    Cl, _ = rq.update_codebooks_chain_bin(X, B, 300, wide=True)
    assert len(Cl) == 4 and Cl[0].shape == (300, 8)
    rq.update_codebooks_chain_bin(Xs, Bs, 256)
    rq.update_codebooks_chain_bin(Xs, Bs, 256, wide=True)
    assert seen == ["u16", "u8", "u16"]
