// rq_ivf_rules.h -- the host arithmetic of an IVF load that touches no device: the id rule and the limits of rq_ivf_build /
// rq_ivf_set_codes / rq_ivf_add* (include/rayuela_hip.h states them), and how a batch is cut into sorted pieces.  Plain C++ with
// no HIP in it, so tests/host/ivf_rules_main.cpp exercises it on the CPU (under sanitizers) as the library compiles it.
#pragma once
#include <cstdint>

namespace rq {

constexpr uint64_t IVF_ID_LIMIT = 0xFFFFFFFFull;   // ids and offsets are uint32; 0xFFFFFFFF marks padding

enum IvfRefusal {
  IVF_OK = 0,
  IVF_NO_ROWS = 1,        // n < 1
  IVF_ID_RANGE = 2,       // id_offset + n > 2^32 - 1
  IVF_ID_ORDER = 3,       // an add whose id_offset lies below the next id
  IVF_ROW_RANGE = 4,      // rows loaded + n > 2^32 - 1
};

// loaded: the rows of the base an add goes behind (0: no base, or a call that replaces it); next_id: the largest id loaded
// plus one (0 for no base).  The checks in the order the entry points report them.
inline IvfRefusal ivf_load_rule(int64_t loaded, uint64_t next_id, int64_t n, uint32_t id_offset) {
  if (n < 1) return IVF_NO_ROWS;
  if ((uint64_t)n + (uint64_t)id_offset > IVF_ID_LIMIT) return IVF_ID_RANGE;
  if (loaded > 0 && (uint64_t)id_offset < next_id) return IVF_ID_ORDER;
  if (loaded > 0 && (uint64_t)loaded + (uint64_t)n > IVF_ID_LIMIT) return IVF_ROW_RANGE;
  return IVF_OK;
}

// a batch of n rows in pieces of `piece` rows (>= 1): the number of pieces, and rows [*r0, *r0 + *cnt) of piece p
inline int64_t ivf_piece_count(int64_t n, int64_t piece) { return n < 1 ? 0 : (n + piece - 1) / piece; }
inline void ivf_piece_span(int64_t n, int64_t piece, int64_t p, int64_t *r0, uint32_t *cnt) {
  *r0 = p * piece;
  const int64_t left = n - *r0;
  *cnt = (uint32_t)(left < piece ? left : piece);
}

}  // namespace rq
