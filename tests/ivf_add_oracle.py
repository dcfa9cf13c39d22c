"""numpy restatement of an ADD to the IVFADC index (include/rayuela_hip.h, "IVFADC": rq_ivf_add / _add_bytes / _add_codes;
DESIGN.md section 4.30).  TEST INFRASTRUCTURE, beside tests/ivf_oracle.py.

A grouped base is (offsets [nlist + 1] int64, ids [n] uint32, codes [n][m]) as ivf_oracle.group returns it.  An add of a batch
(lists [b], codes [b][m], id_offset) gives, list by list: the loaded rows of the list first, in the order they have, then the
batch's rows of that list in arrival order with the ids i + id_offset.  The id rule and the limits are refusal().
"""
import numpy as np

LIMIT = 0xFFFFFFFF        # ids and offsets are uint32; 0xFFFFFFFF marks padding


def next_id(grouped):
    """The largest id loaded plus one; 0 for no base (None, or a base of no rows)."""
    if grouped is None or grouped[1].size == 0:
        return 0
    return int(grouped[1].max()) + 1


def refusal(loaded, nxt, n, id_offset):
    """None when an add of n rows at id_offset behind `loaded` rows with next id `nxt` is accepted, else which rule refuses it, in
    the order the entry points check: "rows" (n < 1), "id_range" (id_offset + n > 2^32 - 1), "id_order" (id_offset below the next
    id), "row_range" (loaded + n > 2^32 - 1).  loaded = 0: a build, which only the first two can refuse."""
    if n < 1:
        return "rows"
    if id_offset < 0 or id_offset + n > LIMIT:
        return "id_range"
    if loaded > 0 and id_offset < nxt:
        return "id_order"
    if loaded > 0 and loaded + n > LIMIT:
        return "row_range"
    return None


def add(grouped, lists, codes, nlist, id_offset):
    """The grouped base after the add; grouped None (no base): the batch alone, ivf_oracle.group's answer."""
    lists = np.asarray(lists, dtype=np.int64)
    codes = np.asarray(codes)
    b = lists.shape[0]
    if grouped is None:
        grouped = (np.zeros(nlist + 1, dtype=np.int64), np.empty(0, dtype=np.uint32), np.empty((0, codes.shape[1]), codes.dtype))
    off_old, ids_old, codes_old = grouped
    assert refusal(ids_old.size, next_id(grouped), b, id_offset) is None
    old_sizes = np.diff(off_old)
    new_sizes = np.bincount(lists, minlength=nlist)
    off_new = np.zeros(nlist + 1, dtype=np.int64)
    off_new[1:] = np.cumsum(old_sizes + new_sizes)
    ids = np.empty(ids_old.size + b, dtype=np.uint32)
    out = np.empty((ids_old.size + b, codes.shape[1]), dtype=codes_old.dtype)
    for l in range(nlist):
        a, k = int(off_new[l]), int(old_sizes[l])
        ids[a:a + k] = ids_old[off_old[l]:off_old[l + 1]]
        out[a:a + k] = codes_old[off_old[l]:off_old[l + 1]]
        rows = np.flatnonzero(lists == l)                        # arrival order
        ids[a + k:off_new[l + 1]] = ((rows + int(id_offset)) & LIMIT).astype(np.uint32)
        out[a + k:off_new[l + 1]] = codes[rows]
    return off_new, ids, out


def chain(pieces, nlist):
    """add() over pieces [(lists, codes, id_offset), ...] from no base; the bases after every piece."""
    grouped, out = None, []
    for lists, codes, id_offset in pieces:
        grouped = add(grouped, lists, codes, nlist, id_offset)
        out.append(grouped)
    return out
