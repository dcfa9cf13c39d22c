"""The kept in-call row order (csrc/rq_order.hip, "the kept order"): a raw-pointer scan keeps the ordered scratch copy of its base
from call to call and proves on the device, byte for byte, that the copy still is the order of the codes it was handed.  Whatever
the cache does, every answer equals the oracle's (ids and distance bits) on a query sample and the SCAN_ORDER = 0 answer on all
queries; rq_order_cache_stats says what the device decided (counts, not clocks)."""
import ctypes as C
import threading

import numpy as np
import pytest

from switch_table import switches

pytestmark = pytest.mark.gpu

SUB, NQ, NQ_ORACLE = 4, 64, 6


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _stats():
    from rayuela_jl_amd import _lib
    return _lib.order_cache_stats()


def _liblib():
    from rayuela_jl_amd import _lib
    return _lib.lib()


def _release():
    from rayuela_jl_amd import _lib
    _lib.check(_lib.lib().rq_release_workspaces())


def _balances(n, m):
    """Does a once-ordered base of this shape get the greedy balance (rq_order_plan, as tests/test_gpu_switches.py reads it)?"""
    from rayuela_jl_amd import _lib
    out = (C.c_int * 14)()
    assert _lib.lib().rq_order_plan(n, m, C.cast(out, C.c_void_p), 14) == 0
    return out[12] != 0


class Base:
    """Codes on the device, tables and queries, and the answers they must give."""

    def __init__(self, n, m, seed, nq=NQ):
        import torch
        import rayuela_jl_amd.synth as synth
        rng = np.random.default_rng(seed)
        self.n, self.m = n, m
        self.codes = synth.random_codes(n, m, seed=seed)
        self.centers = rng.standard_normal((m, 256, SUB)).astype(np.float32)
        self.queries = rng.standard_normal((nq, m * SUB)).astype(np.float32)
        self.cd = torch.from_numpy(self.codes).cuda()
        self.ce = torch.from_numpy(self.centers).cuda()
        self.qd = torch.from_numpy(self.queries).cuda()

    def scan(self, K, cd=None):
        import torch
        from rayuela_jl_amd import device as rqd
        d, i = rqd.linscan(self.cd if cd is None else cd, self.ce, self.qd, K)
        torch.cuda.current_stream().synchronize()
        return d.cpu().numpy(), i.cpu().numpy()

    def check(self, oracle, K, got, codes=None):
        """got == the oracle on the first queries, == the arrival-order scan (SCAN_ORDER = 0) on all of them."""
        import torch
        codes = self.codes if codes is None else codes
        d0, i0 = oracle.linscan_aqd_query(codes, self.centers, self.queries[:NQ_ORACLE], K)
        assert np.array_equal(_bits(got[1][:NQ_ORACLE]), _bits(i0)), "ids differ from the oracle"
        assert np.array_equal(_bits(got[0][:NQ_ORACLE]), _bits(d0)), "distances differ from the oracle"
        with switches(SCAN_ORDER=0):
            d1, i1 = self.scan(K, cd=torch.from_numpy(codes).cuda())
        assert np.array_equal(_bits(got[1]), _bits(i1)), "ids differ from the arrival-order scan"
        assert np.array_equal(_bits(got[0]), _bits(d1)), "distances differ from the arrival-order scan"


@pytest.mark.parametrize("n,m", [(200_000, 8), (1_000_000, 8), (200_000, 16), (1_000_000, 16)])
def test_repeated_calls_build_once_upgrade_once_then_hit(rq, oracle, n, m):
    b = Base(n, m, seed=n + m)
    bal = _balances(n, m)
    if m == 8:
        assert bal == (n == 1_000_000)          # the flagship shape balances, 2e5 rows have no balance in their plan
    with switches(ORDER_MIN_NQ=1):
        for K in (1, 100, 1000):
            _release()
            assert _liblib().rq_scan_orders_in_call(n, NQ, K) == 1
            for _ in range(4):
                b.check(oracle, K, b.scan(K))     # (check() scans with SCAN_ORDER = 0 in between: no ordering, the copy stays)
            st = _stats()
            assert st["consulted"] == 4 and st["uncached"] == 0, st
            assert st["plain_builds"] == 1, st
            assert st["balanced_builds"] == (1 if bal else 0) and st["upgrades"] == st["balanced_builds"], st
            assert st["hits"] == (2 if bal else 3), st


def test_a_batch_that_pays_for_the_balance_builds_it_at_once(rq, oracle):
    """From ORDER_GREEDY_MIN_NQ queries on the first build is balanced, as it always was; nothing is left to upgrade."""
    n, m, K = 1_000_000, 8, 100
    b = Base(n, m, seed=5)
    _release()
    with switches(ORDER_MIN_NQ=1, ORDER_GREEDY_MIN_NQ=32):
        assert _liblib().rq_scan_orders_in_call(n, NQ, K) == 2
        b.check(oracle, K, b.scan(K))
        b.check(oracle, K, b.scan(K))
    st = _stats()
    assert (st["consulted"], st["hits"], st["plain_builds"], st["balanced_builds"], st["upgrades"]) == (2, 1, 0, 1, 0), st


def test_a_short_first_batch_then_large_batches_still_get_the_balance(rq, oracle):
    """A plain copy left by a short first batch is upgraded by the first large batch that hits on it (a batch of ORDER_GREEDY_MIN_NQ
    queries or more balanced its own copy in every call before there was a kept order); a large batch that misses builds balanced."""
    import torch
    n, m, K = 1_000_000, 8, 100
    b = Base(n, m, seed=6)
    _release()
    with switches(ORDER_MIN_NQ=1):
        b.check(oracle, K, b.scan(K))                            # short batch: plain
        st = _stats()
        assert (st["plain_builds"], st["balanced_builds"]) == (1, 0), st
        with switches(ORDER_GREEDY_MIN_NQ=32):                   # NQ = 64 queries now count as a large batch
            assert _liblib().rq_scan_orders_in_call(n, NQ, K) == 2
            for _ in range(3):
                b.check(oracle, K, b.scan(K))
            st = _stats()
            assert (st["consulted"], st["hits"], st["plain_builds"], st["balanced_builds"], st["upgrades"]) == (4, 2, 1, 1, 1), st
            b.cd[7, 0] ^= 0x80
            torch.cuda.current_stream().synchronize()
            b.codes[7, 0] ^= 0x80
            b.check(oracle, K, b.scan(K))
            b.check(oracle, K, b.scan(K))
            st = _stats()
            assert (st["hits"], st["plain_builds"], st["balanced_builds"], st["upgrades"]) == (3, 1, 2, 1), st


def test_one_level_order_is_kept_and_checked_too(rq, oracle):
    """ORDER_TWO_LEVEL = 0: the order_rank / scan / scatter path, gated the same way (its histogram is zeroed only for a rebuild)."""
    import torch
    n, m, K = 200_000, 8, 100
    b = Base(n, m, seed=7)
    _release()
    with switches(ORDER_MIN_NQ=1, ORDER_TWO_LEVEL=0):
        for _ in range(3):
            b.check(oracle, K, b.scan(K))
        st = _stats()
        assert (st["consulted"], st["hits"], st["plain_builds"], st["balanced_builds"]) == (3, 2, 1, 0), st
        b.cd[n - 1, 2] ^= 0x20
        torch.cuda.current_stream().synchronize()
        b.codes[n - 1, 2] ^= 0x20
        b.check(oracle, K, b.scan(K))
        b.check(oracle, K, b.scan(K))
        st = _stats()
        assert (st["hits"], st["plain_builds"]) == (3, 2), st


def test_codes_changed_in_place_are_a_miss_with_the_new_answer(rq, oracle):
    import torch
    n, m, K = 200_000, 8, 100
    b = Base(n, m, seed=77)
    _release()
    with switches(ORDER_MIN_NQ=1):
        b.check(oracle, K, b.scan(K))
        b.scan(K)
        assert (_stats()["plain_builds"], _stats()["hits"]) == (1, 1)
        codes = b.codes.copy()
        builds = 1
        # a byte of the first row, of the last row, of a row of the every-16th sample prefix, and low bits only (the sort key is made
        # of the top bits of the leading bytes: the row keeps its key and its bucket)
        for row, col, xor in [(0, 3, 0x80), (n - 1, m - 1, 0x40), (16 * 5, 0, 0xC0), (12_345, 0, 0x01)]:
            codes[row, col] ^= xor
            b.cd[row, col] = int(codes[row, col])               # the same buffer, rewritten in place
            torch.cuda.current_stream().synchronize()
            b.check(oracle, K, b.scan(K), codes=codes)
            builds += 1
            st = _stats()
            assert (st["plain_builds"], st["hits"], st["balanced_builds"]) == (builds, 1, 0), (row, st)
        b.scan(K)
        assert _stats()["hits"] == 2


def test_same_content_elsewhere_hits_and_other_content_at_the_same_address_does_not(rq, oracle):
    import torch
    n, m, K = 200_000, 8, 100
    b = Base(n, m, seed=78)
    _release()
    with switches(ORDER_MIN_NQ=1):
        b.check(oracle, K, b.scan(K))
        twin = b.cd.clone()
        b.check(oracle, K, b.scan(K, cd=twin))
        st = _stats()
        assert (st["plain_builds"], st["hits"]) == (1, 1), st
        # other rows, fewer of them, at the very same address
        n2 = 150_000
        other = Base(n2, m, seed=79)
        other.centers, other.queries, other.ce, other.qd = b.centers, b.queries, b.ce, b.qd
        b.cd[:n2].copy_(torch.from_numpy(other.codes).cuda())
        view = b.cd[:n2]
        assert view.data_ptr() == b.cd.data_ptr()
        other.check(oracle, K, other.scan(K, cd=view))
        st = _stats()
        assert (st["plain_builds"], st["hits"]) == (2, 1), st
        other.check(oracle, K, other.scan(K, cd=view))
        assert _stats()["hits"] == 2


def test_a_switch_that_shapes_the_order_rebuilds_it(rq, oracle):
    n, m, K = 1_000_000, 8, 100
    b = Base(n, m, seed=80)
    _release()

    def builds(st):
        return st["plain_builds"] + st["balanced_builds"]

    with switches(ORDER_MIN_NQ=1):
        b.scan(K)
        b.check(oracle, K, b.scan(K))
        st = _stats()
        assert (st["plain_builds"], st["balanced_builds"], st["upgrades"], st["hits"]) == (1, 1, 1, 0), st
        for kv in (dict(ORDER_GREEDY=0), dict(ORDER_BITS=11), dict(ORDER_SAMPLE_STRIDE=8)):
            with switches(**kv):
                before = _stats()
                b.check(oracle, K, b.scan(K))
                st = _stats()
                assert builds(st) == builds(before) + 1 and st["hits"] == before["hits"], (kv, before, st)
                if "ORDER_GREEDY" in kv:            # no balance ever: the copy's later uses are plain hits
                    assert st["plain_builds"] == before["plain_builds"] + 1, st
                    b.scan(K)
                    b.check(oracle, K, b.scan(K))
                    st2 = _stats()
                    assert st2["hits"] == st["hits"] + 2 and builds(st2) == builds(st), st2


def test_release_between_calls_rebuilds(rq, oracle):
    n, m, K = 200_000, 8, 100
    b = Base(n, m, seed=81)
    _release()
    with switches(ORDER_MIN_NQ=1):
        b.scan(K)
        b.scan(K)
        assert (_stats()["plain_builds"], _stats()["hits"]) == (1, 1)
        _release()
        assert _stats()["consulted"] == 0
        b.check(oracle, K, b.scan(K))
        st = _stats()
        assert (st["consulted"], st["plain_builds"], st["hits"]) == (1, 1, 0), st


def test_two_streams_and_two_threads_keep_their_own_orders(rq, oracle):
    import torch
    n, m, K = 200_000, 8, 100
    bases = [Base(n, m, seed=90), Base(n, m, seed=91)]
    want = [oracle.linscan_aqd_query(b.codes, b.centers, b.queries[:NQ_ORACLE], K) for b in bases]
    _release()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    errors = []

    def work(t):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(streams[t]):
                for _ in range(4):
                    d, i = bases[t].scan(K)
                    assert np.array_equal(_bits(i[:NQ_ORACLE]), _bits(want[t][1])) and np.array_equal(_bits(d[:NQ_ORACLE]), _bits(want[t][0]))
        except BaseException as e:      # noqa: BLE001 -- reported by the main thread
            errors.append((t, repr(e)))

    with switches(ORDER_MIN_NQ=1):
        threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        st = _stats()
        assert (st["consulted"], st["plain_builds"], st["hits"]) == (8, 2, 6), st
        # one stream, two bases in turn: every call is a miss, every answer right
        _release()
        for _ in range(2):
            for t in range(2):
                d, i = bases[t].scan(K)
                assert np.array_equal(_bits(i[:NQ_ORACLE]), _bits(want[t][1])) and np.array_equal(_bits(d[:NQ_ORACLE]), _bits(want[t][0]))
        st = _stats()
        assert (st["consulted"], st["plain_builds"], st["hits"], st["balanced_builds"]) == (4, 4, 0, 0), st


def test_other_calls_in_between_leave_the_kept_order_alone(rq, oracle):
    """A k = 10000 call (scans the arrival order), an LSQ scan (orders nothing) and a host-pointer call (orders into an allocation of
    its own) between cached calls: the cached calls stay hits and every answer stays right."""
    import torch
    from rayuela_jl_amd import device as rqd
    n, m, K = 200_000, 8, 100
    b = Base(n, m, seed=95)
    rng = np.random.default_rng(96)
    books = torch.from_numpy(rng.standard_normal((m * 256, m * SUB)).astype(np.float32)).cuda()
    norms = torch.from_numpy(rng.random(n).astype(np.float32)).cuda()
    _release()
    with switches(ORDER_MIN_NQ=1):
        assert _liblib().rq_scan_orders_in_call(n, NQ, 10_000) == 0
        lsq0 = [t.cpu().numpy() for t in rqd.linscan_aq(b.cd, books, b.qd, K, dbnorms=norms)]
        big0 = b.scan(10_000)
        host0 = rq.linscan_aqd_query(b.codes, b.centers, b.queries[:NQ_ORACLE], K)
        b.check(oracle, K, b.scan(K))
        for _ in range(2):
            big = b.scan(10_000)
            assert np.array_equal(_bits(big[0]), _bits(big0[0])) and np.array_equal(_bits(big[1]), _bits(big0[1]))
            b.check(oracle, K, b.scan(K))
            lsq = [t.cpu().numpy() for t in rqd.linscan_aq(b.cd, books, b.qd, K, dbnorms=norms)]
            assert np.array_equal(_bits(lsq[0]), _bits(lsq0[0])) and np.array_equal(_bits(lsq[1]), _bits(lsq0[1]))
            b.check(oracle, K, b.scan(K))
            host = rq.linscan_aqd_query(b.codes, b.centers, b.queries[:NQ_ORACLE], K)
            assert np.array_equal(_bits(host[0]), _bits(host0[0])) and np.array_equal(_bits(host[1]), _bits(host0[1]))
            b.check(oracle, K, b.scan(K))
    d0, i0 = oracle.linscan_aqd_query(b.codes, b.centers, b.queries[:NQ_ORACLE], 10_000)
    assert np.array_equal(_bits(big0[1][:NQ_ORACLE]), _bits(i0)) and np.array_equal(_bits(big0[0][:NQ_ORACLE]), _bits(d0))
    st = _stats()
    assert (st["consulted"], st["plain_builds"], st["hits"], st["uncached"]) == (7, 1, 6, 0), st


def test_snapshot_over_the_scratch_cap_orders_uncached(rq, oracle):
    """ORDER_MAX_SCRATCH_MB counts the snapshot: copy + perm + key scratch fit (n * (mp + 8)), the snapshot does not -> every call orders
    its scratch copy as before, nothing is kept, and rq_scan_orders_in_call keeps its answer."""
    n, m, K = 200_000, 8, 100
    b = Base(n, m, seed=97)
    _release()
    with switches(ORDER_MIN_NQ=1, ORDER_MAX_SCRATCH_MB=4):       # 3.2 MB without the snapshot, 4.8 MB with it
        assert _liblib().rq_scan_orders_in_call(n, NQ, K) == 1
        for _ in range(2):
            b.check(oracle, K, b.scan(K))
        st = _stats()
        assert (st["consulted"], st["uncached"]) == (0, 2), st
