"""CPU (host code only, and hipcc cross-compiles): the planner's view of the bulk top-k path (k > RQ_MAX_K) and the
generated code of its kernels.

1. rq_scan_plan reports bit 2 of its flags (`scan_plan(...)["bulk"]`) exactly when k > RQ_MAX_K = 65536, for every tiled
   row width and up to n = 2^31 - 1 rows; below the cap the plan is the candidate-buffer scan's, field for field as
   before the bulk path existed (pinned below from the planner of that version).
2. No kernel of rq_bulk.hip touches scratch memory (kernel-resource-usage: ScratchSize 0)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
RQ_MAX_K = 65536

FIELDS = ("qg", "groups", "whole", "slices", "rows_per_slice", "grid", "cap", "flags")
# (n, nq, m, d, k) -> the plan of the candidate-buffer scan, as the planner computed it before the bulk path
PINNED = {
    (1000000, 1000, 8, 128, 10000): (8, 125, 0, 3, 335872, 375, 93968, 1),
    (1000000, 1000, 8, 128, 65536): (8, 125, 125, 1, 1007616, 125, 231424, 1),
    (1000000, 100, 16, 128, 65536): (8, 13, 13, 1, 1003520, 13, 231424, 1),
    (70000, 9, 4, 32, 65536): (8, 2, 2, 1, 81920, 2, 231424, 1),
    (2147483647, 100, 8, 128, 65536): (8, 13, 0, 39, 55066624, 507, 231424, 1),
    (1000000, 10000, 8, 128, 1000): (8, 1250, 1250, 1, 1007616, 512, 72584, 0),
    (1000000, 100, 2, 8, 65536): (8, 13, 13, 1, 1015808, 13, 231424, 1),
    (1000000, 100, 64, 256, 65536): (2, 50, 50, 1, 1000448, 50, 182272, 1),
}


@pytest.fixture(scope="module")
def lib():
    import rayuela_jl_amd._lib as L
    return L


@pytest.mark.parametrize("n", [1000000, 2 ** 31 - 1])
@pytest.mark.parametrize("m", [2, 8, 16, 64])
def test_bulk_bit_is_set_exactly_above_the_cap(lib, m, n):
    d = 4 * m
    below = lib.scan_plan(n, 100, m, d, RQ_MAX_K)
    above = lib.scan_plan(n, 100, m, d, RQ_MAX_K + 1)
    assert below["bulk"] == 0 and (below["flags"] & 4) == 0, below
    assert above["bulk"] == 1 and (above["flags"] & 4) == 4, above
    assert above["xcd"] == 0 and above["bigk"] == 1, above       # bits 0 and 1 keep their meaning
    assert above["slices"] == 1 and above["rows_per_slice"] == n and above["whole"] == above["groups"], above
    # cap = queries per bulk batch: at 1e6 rows a batch holds many queries, at 2^31 - 1 rows not even one (8 bytes a row)
    assert (above["cap"] >= 1) == (n == 1000000), above
    assert lib.scan_plan(n, 100, m, d, n)["bulk"] == 1


@pytest.mark.parametrize("shape", sorted(PINNED))
def test_plan_below_the_cap_is_unchanged(lib, shape):
    n, nq, m, d, k = shape
    p = lib.scan_plan(n, nq, m, d, k)
    assert tuple(p[f] for f in FIELDS) == PINNED[shape], (shape, p)
    assert p["bulk"] == 0


@pytest.fixture(scope="module")
def bulk_usage():
    if not os.path.isfile(HIPCC):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "rayuela.jl_amd", "csrc", "rq_bulk.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-c",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", src, "-o", os.devnull],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    usage = {}
    name = None
    for ln in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
        if m and name:
            usage[name] = int(m.group(1))
    return usage


def test_bulk_kernels_do_not_spill(bulk_usage):
    names = sorted(bulk_usage)
    # every stage is there: the distance kernel for all six row widths (with and without the row bias) and the select / sort
    keys = [n for n in names if "adc_bulk_keys_kernel" in n]
    assert len(keys) == 12, names
    for stage in ("bulk_hist_kernel", "bulk_pick_kernel", "bulk_compact_kernel", "bulk_sort_hist_kernel",
                  "bulk_sort_scan_kernel", "bulk_sort_scatter_kernel", "bulk_unpack_kernel"):
        assert any(stage in n for n in names), (stage, names)
    spills = {n: s for n, s in bulk_usage.items() if s}
    assert not spills, spills
