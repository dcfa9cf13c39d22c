"""CPU: the switch table (tests/switch_table.py) against the keys the library reads, the "unset" semantics of rq_reset_tuning,
and rq_order_plan's balance flag against the launch's own predicate (host-only readouts: no device needed)."""
import ctypes as C
import glob
import os
import re

import pytest

from switch_table import SWITCHES, switches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayuela.jl_amd", "csrc")


def _code_keys():
    """key -> set of defaults at its call sites `tuning("KEY", default)`."""
    keys = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        src = open(path).read()
        for k, dflt in re.findall(r'\btuning\("([A-Z0-9_]+)",\s*([^()]*(?:\([^()]*\))?[^()]*)\)', src):
            keys.setdefault(k, set()).add(eval(dflt.strip(), {}))
    return keys


def test_every_key_the_code_reads_is_in_the_table_with_its_default():
    keys = _code_keys()
    assert len(keys) == 69, sorted(keys)
    assert sorted(set(keys) - set(SWITCHES)) == [], "switches missing from tests/switch_table.py"
    assert sorted(set(SWITCHES) - set(keys)) == [], "table entries the code no longer reads"
    for k, dflts in keys.items():
        assert len(dflts) == 1, (k, dflts)                    # one default across every call site
        assert dflts == {SWITCHES[k]["default"]}, (k, dflts, SWITCHES[k]["default"])


def test_every_entry_is_swept_tested_elsewhere_or_explained():
    for k, e in SWITCHES.items():
        kinds = [x for x in ("values", "tested_in", "reason") if x in e]
        assert len(kinds) == 1, (k, kinds)
        if "values" in e:
            assert e["values"] and e["default"] not in e["values"] and e.get("workload"), k
            # what tells the switched path from the default one -- or, in the note, why nothing can
            assert e.get("readout") in ("orders", "plan", "kernel", "order_plan", "encode_kernel") or \
                str(e.get("readout")).startswith("stats:") or "readout" in e.get("note", ""), k
        else:
            assert "readout" not in e, k
        if "tested_in" in e:
            path, name = e["tested_in"].split("::")
            assert re.search(r"^def %s\(" % name, open(os.path.join(ROOT, path)).read(), re.M), (k, e["tested_in"])
        if "reason" in e:
            assert len(e["reason"]) > 20, k


def test_integration_doc_names_only_keys_the_code_reads():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("## 6."):]
    sec = sec[:sec.index("\n## ", 4)] if "\n## " in sec[4:] else sec
    named = set()
    for row in re.findall(r"^\| (.*?) \|", sec, re.M):
        named |= set(re.findall(r"`(?:RQ_)?([A-Z][A-Z0-9_]+)`", row))
    named -= {"RAYUELA_HIP_DEVICES"}                           # an environment variable of the shims, not a tuning key
    assert len(named) > 30, named
    keys = _code_keys()
    assert sorted(named - set(keys)) == [], "INTEGRATION.md section 6 names keys the code does not read"


def _scan_plan():
    from rayuela_jl_amd import _lib
    return _lib.scan_plan(1_000_000, 8, 8, 128, 10_000)


def _order(n, m):
    from rayuela_jl_amd import _lib
    out = (C.c_int * 14)()
    assert _lib.lib().rq_order_plan(n, m, C.cast(out, C.c_void_p), 14) == 0
    return list(out)


def test_reset_returns_a_switch_to_its_default(monkeypatch):
    """set -> the host-only plans move; reset -> they are the default's again, and RQ_<KEY> from the environment rules again
    (a value stored by set_tuning hides it -- what restoring 'by value' used to do)."""
    from rayuela_jl_amd import _lib
    plan0, order0 = _scan_plan(), _order(1_000_000, 8)
    with switches(SCAN_SS_MIN_K=1 << 20, ORDER_GREEDY=0, ORDER_BITS=20):
        assert _scan_plan()["bigk"] == 0 and plan0["bigk"] == 1
        assert _order(1_000_000, 8)[8] == 20
    assert _scan_plan() == plan0 and _order(1_000_000, 8) == order0
    monkeypatch.setenv("RQ_ORDER_BITS", "14")
    assert _order(1_000_000, 8)[8] == 14
    try:
        _lib.set_tuning("ORDER_BITS", 0)
        assert _order(1_000_000, 8) == order0             # a stored value hides the environment ...
        _lib.reset_tuning("ORDER_BITS")
        assert _order(1_000_000, 8)[8] == 14              # ... a reset does not
        _lib.set_tuning("ORDER_GREEDY", 0)
        _lib.set_tuning("ORDER_BITS", 20)
        _lib.reset_tuning(None)                           # NULL: every key
        assert _order(1_000_000, 8)[8] == 14
    finally:
        _lib.reset_tuning("ORDER_BITS")
        _lib.reset_tuning("ORDER_GREEDY")
    monkeypatch.delenv("RQ_ORDER_BITS")
    assert _order(1_000_000, 8) == order0
    _lib.reset_tuning("NOT_A_KEY")                        # resetting what was never set is fine


def test_the_table_holds_every_key_at_once():
    """Setting every switch of the table in one process (69 keys) used to fail with 'too many tuning keys' past 64."""
    with switches(**{k: e["default"] for k, e in SWITCHES.items()}):
        pass
    with pytest.raises(KeyError):
        with switches(NOT_A_KEY=1):
            pass


# ---- rq_order_plan against order_rows_launch's predicate --------------------------------------------------------------------
def _launch_balances(n, m):
    """order_rows_launch balances exactly where order_key_bits gave up a table's 3 bits for it: the key with the balance
    allowed is 3 bits shorter than the plain key (ORDER_GREEDY = 0 leaves the full budget)."""
    with switches(ORDER_GREEDY=0):
        plain = _order(n, m)[8]
    return _order(n, m)[8] == plain - 3


def test_order_plan_reports_the_plain_sort_at_3e5_rows():
    """n = 3e5, m = 8: the full budget is 13 bits, too short for the balance, so the launch runs order_fine_kernel; the plan
    used to ask order_greedy_plan about a 16-bit budget and report 4 tables / 16 wavefronts."""
    p = _order(300_000, 8)
    assert p[8] == 13 and p[12] == 0 and p[13] == 0
    assert not _launch_balances(300_000, 8)


@pytest.mark.parametrize("m", [8, 16])
def test_order_plan_balance_flag_equals_the_launch_predicate(m):
    ns = list(range(200_000, 1_200_000, 5_000)) + list(range(1_200_000, 4_000_001, 100_000)) + [4_400_000, 4_500_000, 6_000_000]
    on = []
    for n in ns:
        p = _order(n, m)
        assert (p[12] != 0) == _launch_balances(n, m), (n, m, p)
        assert (p[12] != 0) == (p[13] != 0), (n, m, p)
        if p[12]:
            assert p[12] == (4 if m == 8 else 12), (n, m, p)
        on.append(p[12] != 0)
    # on-device balancing starts at ~7.9e5 rows (~7.4e5 sorted rows) and stops where a coarse bucket outgrows the LDS list
    first = ns[on.index(True)]
    assert 780_000 <= first <= 800_000, first
    assert on[ns.index(1_000_000)] and on[ns.index(4_000_000)]
    assert not on[ns.index(6_000_000)]
    if m == 16:
        assert not on[ns.index(4_500_000)]
