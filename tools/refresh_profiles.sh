#!/bin/bash
# Profile round on a GPU box, collect into profiles/, then re-run the six bench lines that replay traffic WITH the fresh replay
# files in place (they are bound to the library build) and store those lines too.
#   GPU_RUN='<command that runs its one argument, a shell line, in a copy of this tree on a GPU box and copies $OUT back>' \
#   OUT=<the folder tools/profile_round6.sh and tools/collect_profiles.py write and read> bash tools/refresh_profiles.sh
set -e
cd "$(dirname "$0")/.."
: "${GPU_RUN:?set GPU_RUN}" "${OUT:?set OUT}"
rm -rf "$OUT/r6" "$OUT/r6b"
$GPU_RUN "rm -rf $OUT/r6; bash tools/profile_round6.sh > $OUT/r6_profile.log 2>&1; tail -2 $OUT/r6_profile.log"
python tools/collect_profiles.py r6 | head -12
B="python bench.py --full"
$GPU_RUN "mkdir -p $OUT/r6b; $B > $OUT/r6b/bench_pq.json 2>/dev/null; $B --workload opq > $OUT/r6b/bench_opq.json 2>/dev/null; $B --workload deep > $OUT/r6b/bench_deep.json 2>/dev/null; $B --k 10000 --no-cpu > $OUT/r6b/bench_pq_k10000.json 2>/dev/null; $B --workload sift1b --steps 3 --warmup 1 > $OUT/r6b/bench_sift1b_1gpu.json 2>/dev/null; $B --workload sift1b --rows 125000000 --steps 5 --warmup 1 --no-cpu > $OUT/r6b/bench_sift1b_shard.json 2>/dev/null; echo done"
OUT="$OUT" python - <<'PY'
import json, os
for w in ("pq", "opq", "deep", "pq_k10000", "sift1b_1gpu", "sift1b_shard"):
    d = json.loads(open(os.path.join(os.environ["OUT"], "r6b", "bench_%s.json" % w)).read().strip().splitlines()[-1])
    r = d["roofline"]; e = d.get("encode") or {}; er = e.get("roofline") or {}
    print(w, d["ms_per_step"], "kernel", r.get("kernel_ms"), "frac", r["frac"], "traffic", r["traffic"], "| enc", e.get("ms_per_step"), er.get("bound"), er.get("frac"))
    open("profiles/r6_bench_%s.json" % w, "w").write(json.dumps(d) + "\n")
PY
