// A stand-alone host program over rayuela.jl_amd/csrc/rq_ivf_rules.h: the id rule, the limits and the piece arithmetic of an IVF
// load, as the library compiles them, with no device and no HIP.  tests/test_ivf_add_oracle.py builds it (with
// -fsanitize=address,undefined where the host compiler has them) and holds its answers to tests/ivf_add_oracle.py.
//   stdin:  lines "loaded next_id n id_offset"      stdout: one refusal code per line (IvfRefusal)
// Before it reads, it walks the piece arithmetic over a grid of (n, piece) and exits 2 on a piece that does not tile the batch.
#include <cinttypes>
#include <cstdio>

#include "rq_ivf_rules.h"

static int pieces_ok() {
  const int64_t ns[] = {1, 2, 255, 256, 257, 3000, (int64_t)1 << 25, ((int64_t)1 << 25) + 1, 0xFFFFFFFFll};
  const int64_t ps[] = {1, 2, 512, 999, 3000, (int64_t)1 << 25};
  for (int64_t n : ns)
    for (int64_t piece : ps) {
      const int64_t P = rq::ivf_piece_count(n, piece);
      if (P > (1 << 20)) continue;                       // (a grid, not a stress run)
      int64_t at = 0;
      for (int64_t p = 0; p < P; ++p) {
        int64_t r0;
        uint32_t cnt;
        rq::ivf_piece_span(n, piece, p, &r0, &cnt);
        if (r0 != at || cnt < 1 || (int64_t)cnt > piece) return 0;
        at += cnt;
      }
      if (at != n) return 0;
    }
  return rq::ivf_piece_count(0, 512) == 0;
}

int main() {
  if (!pieces_ok()) { fprintf(stderr, "pieces do not tile the batch\n"); return 2; }
  long long loaded, n;
  unsigned long long next_id, id_offset;
  while (scanf("%lld %llu %lld %llu", &loaded, &next_id, &n, &id_offset) == 4) {
    if (id_offset > 0xFFFFFFFFull) return 3;             // the C ABI takes a uint32
    printf("%d\n", (int)rq::ivf_load_rule((int64_t)loaded, (uint64_t)next_id, (int64_t)n, (uint32_t)id_offset));
  }
  return 0;
}
