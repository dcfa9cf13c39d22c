"""CPU: the restatement of an add to the IVFADC index (tests/ivf_add_oracle.py) against the restated build (tests/ivf_oracle.py),
the argument checks of IvfIndex.add / add_codes (rayuela_jl_amd/IVF.py), which raise before the library is called, and the
piecewise file readers ivf_add_bvecs / ivf_add_fvecs (rayuela_jl_amd/xvecs.py) against a stub index."""
import numpy as np
import pytest

import ivf_add_oracle as ivfa
import ivf_oracle as ivf
from test_gpu_ivf import _data, N

LIMIT = 0xFFFFFFFF


def _equal(got, want, what=""):
    for g, w, name in zip(got, want, ("offsets", "ids", "codes")):
        assert np.array_equal(g, w), (name, what)


def _cuts(nlist):
    rng = np.random.default_rng(nlist)
    a, b = sorted(rng.choice(np.arange(1, N), 2, replace=False).tolist())
    return [(1, 2), (1500, 2999), (2999, 3000), (a, b), (40, 90)]


@pytest.mark.parametrize("kind", ["sift", "gauss"])
@pytest.mark.parametrize("nlist", [1, 7, 37, 300])
def test_chained_adds_equal_the_build_of_the_concatenation(oracle, kind, nlist):
    X, Q, centers, _ = _data(kind, nlist=nlist)
    for by_residual in (True, False):
        whole, (lists, _, codes) = ivf.build(X, Q, centers, by_residual, id_offset=11)
        for a, b in _cuts(nlist):
            bounds = [0, a, b, N] if b < N else [0, a, N]
            first, _ = ivf.build(X[:a], Q, centers, by_residual, id_offset=11)
            grouped = first
            for lo, hi in zip(bounds[1:-1], bounds[2:]):
                _, (pl, _, pc) = ivf.build(X[lo:hi], Q, centers, by_residual)
                assert np.array_equal(pl, lists[lo:hi]) and np.array_equal(pc, codes[lo:hi])    # a row's list and codes are its own
                grouped = ivfa.add(grouped, pl, pc, nlist, 11 + lo)
            _equal(grouped, whole, (kind, nlist, by_residual, a, b))
            assert ivfa.next_id(grouped) == 11 + N
            if nlist == 300 and (a, b) == (40, 90):        # lists without a row in the loaded part, and others without one in the batch
                part = ivfa.add(first, lists[40:90], codes[40:90], nlist, 11 + 40)
                old, new = np.diff(first[0]), np.bincount(lists[40:90], minlength=nlist)
                assert ((old == 0) & (new > 0)).any() and ((old > 0) & (new == 0)).any() and ((old == 0) & (new == 0)).any()
                assert np.array_equal(np.diff(part[0]), old + new)


def test_chain_from_no_base_is_the_group_of_the_batch():
    rng = np.random.default_rng(3)
    lists, codes = rng.integers(0, 9, 200), rng.integers(0, 256, (200, 4)).astype(np.uint8)
    _equal(ivfa.add(None, lists, codes, 9, 77), ivf.group(lists, codes, 9, 77))
    assert ivfa.next_id(None) == 0


@pytest.mark.parametrize("nlist", [1, 7, 300])
def test_gaps_in_id_offset_equal_the_group_with_the_explicit_ids(nlist):
    rng = np.random.default_rng(nlist + 5)
    n = 900
    lists, codes = rng.integers(0, nlist, n), rng.integers(0, 256, (n, 5)).astype(np.uint8)
    if nlist == 300:
        lists[lists % 3 == 0] = 299          # runs of empty lists, the last list populated
    bounds = [0, 1, 250, 251, 600, n]
    offsets = [5, 6, 1000, 1001, (1 << 31) + 9]           # the second piece continues without a gap, the others leave one
    pieces = [(lists[lo:hi], codes[lo:hi], off) for lo, hi, off in zip(bounds[:-1], bounds[1:], offsets)]
    explicit = np.concatenate([np.arange(hi - lo, dtype=np.int64) + off for lo, hi, off in zip(bounds[:-1], bounds[1:], offsets)])
    bases = ivfa.chain(pieces, nlist)
    for i, hi in enumerate(bounds[1:]):
        g = ivf.group(lists[:hi], codes[:hi], nlist)
        _equal(bases[i], (g[0], explicit[g[1]].astype(np.uint32), g[2]), (nlist, hi))
    for l in range(nlist):                   # the invariant the search rests on: ids ascend inside a list
        run = bases[-1][1][bases[-1][0][l]:bases[-1][0][l + 1]].astype(np.int64)
        assert np.all(np.diff(run) > 0)
    assert ivfa.next_id(bases[-1]) == offsets[-1] + n - 600


RULE_CASES = [
    # loaded, next id, n, id_offset, the refusal
    (0, 0, 0, 0, "rows"),
    (0, 0, 1, 0, None),
    (0, 0, 10, LIMIT - 10, None),
    (0, 0, 10, LIMIT - 9, "id_range"),
    (0, 0, 5, 1 << 31, None),                          # no base: any id_offset (an add is a build)
    (100, 500, 1, 499, "id_order"),
    (100, 500, 1, 500, None),
    (100, 500, 1, 7000, None),                         # a gap
    (100, LIMIT - 1, 1, LIMIT - 1, None),              # ends exactly at id 2^32 - 2
    (100, LIMIT - 1, 2, LIMIT - 1, "id_range"),
    (100, 500, 3, LIMIT - 2, "id_range"),
    (100, 500, 0, 600, "rows"),
    (LIMIT - 3, LIMIT - 3, 3, LIMIT - 3, None),
    (LIMIT - 3, 10, 4, 20, "row_range"),
    (LIMIT - 3, 10, 4, 5, "id_order"),                 # the id rule is reported before the row limit
]


def test_refusals_of_the_restatement_and_of_the_mirror(rq):
    from rayuela_jl_amd.IVF import IvfIndex
    for loaded, nxt, n, id_offset, want in RULE_CASES:
        assert ivfa.refusal(loaded, nxt, n, id_offset) == want, (loaded, nxt, n, id_offset)
        ix = IvfIndex._unbound(nlist=4, d=12, m=4)
        ix.n, ix.next_id = loaded, nxt
        if want is None:
            assert ix._check_add(n, id_offset) == id_offset
        else:
            with pytest.raises(ValueError):
                ix._check_add(n, id_offset)
    ix = IvfIndex._unbound(nlist=4, d=12, m=4)
    assert ix._check_add(3, None) == 0                  # None: the next id
    ix.n, ix.next_id = 10, 1234
    assert ix._check_add(3, None) == 1234
    with pytest.raises(ValueError, match="1233.*1234"):  # the message names both numbers
        ix._check_add(3, 1233)


def test_mirror_argument_checks_of_add_raise_before_the_library(rq):
    from rayuela_jl_amd.IVF import IvfIndex
    ix = IvfIndex._unbound(nlist=4, d=12, m=4)
    ix.n, ix.next_id = 10, 50
    X = np.zeros((3, 12), dtype=np.float32)
    for bad in (X[:, :8], X.astype(np.uint8)[:, :8], X[0]):          # wrong d, float and byte rows; not a matrix
        with pytest.raises(ValueError):
            ix.add(bad)
    for dtype in (np.float64, np.int32, np.int8, np.float16):        # neither float32 nor uint8
        with pytest.raises(TypeError):
            ix.add(X.astype(dtype))
        with pytest.raises(TypeError):
            ix.build(X.astype(dtype))
    for rows in (X, X.astype(np.uint8)):
        with pytest.raises(ValueError):
            ix.add(rows, id_offset=49)                               # below the next id
        with pytest.raises(ValueError):
            ix.add(rows, id_offset=LIMIT - 2)                        # id_offset + n = 2^32
        with pytest.raises(ValueError):
            ix.add(rows[:0])
        with pytest.raises(ValueError):
            ix.build(rows, id_offset=LIMIT - 2)
    ix.n = LIMIT - 2
    with pytest.raises(ValueError):
        ix.add(X, id_offset=60)                                      # rows loaded + n past 2^32 - 1
    B = np.zeros((3, 4), dtype=np.uint8)
    with pytest.raises(ValueError):
        ix.add_codes(np.array([0, 1, 2]), B, id_offset=60)
    ix.n = 10
    with pytest.raises(ValueError):
        ix.add_codes(np.array([0, 4, 1]), B)                         # list id out of range
    with pytest.raises(ValueError):
        ix.add_codes(np.array([0, -1, 1]), B)
    with pytest.raises(ValueError):
        ix.add_codes(np.array([0, 1, 2]), B[:, :3])
    with pytest.raises(ValueError):
        ix.add_codes(np.array([0, 1]), B)
    with pytest.raises(ValueError):
        ix.add_codes(np.array([0.0, 1.0, 2.0]), B)
    with pytest.raises(ValueError):
        ix.add_codes(np.array([0, 1, 2]), B, id_offset=49)
    with pytest.raises(ValueError):
        ix.add_codes(np.array([0, 1, 2]), B, id_offset=LIMIT - 2)
    wide = IvfIndex._unbound(nlist=4, d=96, m=48)
    with pytest.raises(ValueError):
        wide.add(np.zeros((3, 96), dtype=np.float32))                # add encodes: m <= 32 (add_codes takes codes)
    assert (ix.n, ix.next_id) == (10, 50) and (wide.n, wide.next_id) == (0, 0)       # a refused call changes nothing


class _Stub:
    """What ivf_add_bvecs / ivf_add_fvecs see of an index: d and add(); records (rows, id_offset, dtype, first and last row)."""

    def __init__(self, d):
        self.d, self.calls = d, []

    def add(self, X, id_offset=None):
        self.calls.append((X.shape[0], id_offset, X.dtype, X[0].copy(), X[-1].copy()))


@pytest.mark.parametrize("form", ["bvecs", "fvecs"])
def test_file_readers_add_every_piece_at_its_file_position(tmp_path, form):
    from rayuela_jl_amd import xvecs
    n, d = 23, 6
    rng = np.random.default_rng(8)
    if form == "bvecs":
        X = rng.integers(0, 256, (n, d)).astype(np.uint8)
        write, run = xvecs.bvecs_write, xvecs.ivf_add_bvecs
    else:
        X = rng.standard_normal((n, d)).astype(np.float32)
        write, run = xvecs.fvecs_write, xvecs.ivf_add_fvecs
    path = str(tmp_path / ("x." + form))
    write(X, path)
    for bounds, a, b in ((None, 1, n), (10, 1, 10), ((4, 17), 4, 17), ((n, n), n, n), ((1, 1), 1, 1)):
        for per in (1, 5, 7, 14, n, 1 << 20):
            ix = _Stub(d)
            assert run(ix, path, bounds=bounds, rows_per_read=per) == b - a + 1
            at = a - 1                      # ids are ZERO-based file positions
            for rows, id_offset, dtype, first, last in ix.calls:
                assert id_offset == at and dtype == X.dtype and 1 <= rows <= per
                assert np.array_equal(first, X[at]) and np.array_equal(last, X[at + rows - 1])
                at += rows
            assert at == b and len(ix.calls) == -(-(b - a + 1) // per)
    for bounds in ((0, 3), (5, n + 1), (7, 6), n + 1):
        ix = _Stub(d)
        with pytest.raises(ValueError):
            run(ix, path, bounds=bounds)
        assert ix.calls == []
    with pytest.raises(ValueError):
        run(_Stub(d), path, rows_per_read=0)
    ix = _Stub(d + 1)                       # the file's d is not the index's: refused before anything is added
    with pytest.raises(ValueError):
        run(ix, path)
    assert ix.calls == []


def test_the_librarys_rule_header_on_the_host_equals_the_restatement(tmp_path):
    """rayuela.jl_amd/csrc/rq_ivf_rules.h is plain C++ with no HIP in it: tests/host/ivf_rules_main.cpp is built around it as a
    stand-alone program, with the address and undefined-behaviour sanitizers where the host compiler links them, and answers the
    rule cases above as the restatement does; it checks the piece arithmetic of a batch itself before it reads."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "ivf_rules")
    base = [cxx, "-std=c++17", "-O1", "-g", "-I" + os.path.join(root, "rayuela.jl_amd", "csrc"),
            os.path.join(root, "tests", "host", "ivf_rules_main.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:      # a compiler without the sanitizer runtimes
        subprocess.run(base, check=True, capture_output=True)
    codes = {0: None, 1: "rows", 2: "id_range", 3: "id_order", 4: "row_range"}
    cases = [c for c in RULE_CASES if 0 <= c[3] <= LIMIT]
    rng = np.random.default_rng(12)
    edge = [0, 1, 2, 1000, (1 << 31) - 1, 1 << 31, LIMIT - 2, LIMIT - 1, LIMIT]
    for _ in range(400):
        loaded = int(rng.choice(edge))
        cases.append((loaded, int(rng.choice(edge)) if loaded else 0, int(rng.choice(edge + [-1, 1 << 33])), int(rng.choice(edge)), None))
    text = "".join("%d %d %d %d\n" % c[:4] for c in cases)
    run = subprocess.run([exe], input=text.encode(), capture_output=True)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    got = [codes[int(x)] for x in run.stdout.split()]
    assert got == [ivfa.refusal(*c[:4]) for c in cases]
    assert {None, "rows", "id_range", "id_order", "row_range"} <= set(got)
