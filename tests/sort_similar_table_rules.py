"""-sort-similar over a table of pair scores (include/cbird_hip.h, cbh_sort_similar_table), as a plain model: the loop of
src/main.cpp:1523-1580 written out pass by pass, with the candidate rule of a table.

The score of (needle r, candidate c) is table[r][c], 0xFFFF = no match; rows and columns are in the CALLER's item order,
as the C-ABI takes them.  A candidate is unsorted, in the index and has a score; candidates order by (score, id); the
first max_matches; of those, path_mode and filter_parent; accepted iff 1 + kept > min_matches; the answer is the first
kept.  A query is one numpy pass over the row; the loop is written out pass by pass, and only its end is closed-form: a
whole i iteration without an insert means that every later pass fails."""
import numpy as np

NO_MATCH = 0xFFFF


def table_model(table, ids, min_matches=1, max_matches=5, in_index=None, dir_id=None, under=None, filter_parent=False,
                path_mode=0, look_behind=5):
    """(ids in sorted order, queries, notFound, behind) of one selection given in selection order"""
    ids = np.asarray(ids, np.int64)
    n = len(ids)
    if n < 2:
        return [int(i) for i in ids], 0, 0, 0
    table = np.asarray(table).reshape(n, n)
    # the candidates of any query: unsorted and in the index (the needle is sorted, so it is never among them)
    avail = np.ones(n, bool) if in_index is None else np.asarray(in_index, bool).copy()
    avail[0] = False
    order, queries, not_found, behind = [0], 0, 0, 0

    def ask(needle):
        row = table[needle]
        cand = np.flatnonzero(avail & (row != NO_MATCH))
        cand = cand[np.lexsort((ids[cand], row[cand]))][:max_matches]  # by (score, id), the first max_matches
        kept = []
        for c in cand:
            if path_mode and bool(under[c]) != (path_mode == 1):
                continue
            if filter_parent and dir_id[c] == dir_id[needle]:
                continue
            kept.append(int(c))
        return kept[0] if kept and 1 + len(kept) > min_matches else None

    for i in range(n - 1):
        inserted, j = False, 0
        while j < min(look_behind, len(order)):  # the bound is read again on every pass
            got = ask(order[len(order) - 1 - j])
            if got is None:
                not_found += 1
            else:
                order.insert(len(order) - j, got)
                avail[got] = False
                inserted = True
                behind += j > 0
            queries += 1
            j += 1
        if not inserted:  # nothing can change any more: the remaining iterations fail pass by pass
            rest = (n - 2 - i) * min(look_behind, len(order))
            queries, not_found = queries + rest, not_found + rest
            break
    return [int(ids[k]) for k in order], queries, not_found, int(behind)


def hamming_table(hashes, thresh):
    """the table the 64-bit chain sees with max_thresh 0: popcount(a ^ b), `no match` at or above the threshold and in
    the rows of needles without a hash (src/dcthashindex.cpp:196-200)"""
    h = np.asarray(hashes, np.uint64)
    x = h[:, None] ^ h[None, :]
    d = np.zeros(x.shape, np.int64)
    for b in range(64):
        d += ((x >> np.uint64(b)) & np.uint64(1)).astype(np.int64)
    t = np.where(d < thresh, d, NO_MATCH).astype(np.uint16)
    t[h == 0, :] = NO_MATCH
    return t


def color_table(needles, entries, np_scores, int_scores):
    """uint16 [n, n]: int(ColorDescriptor::distance(needle r, entry c)), 0xFFFF where it is FLT_MAX"""
    s = int_scores(np_scores(needles, entries))
    assert s.max() < NO_MATCH
    return np.where(s < 0, NO_MATCH, s).astype(np.uint16)
