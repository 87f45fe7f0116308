"""CPU: tests/sort_similar_table_rules.py, the plain model of -sort-similar over a table of scores, against the two
restatements of the reference's loop that exist already -- model() of tests/test_sort_similar.py on Hamming tables (the
threshold applied to the table, max_thresh 0) and database._sort_similar_loop driven by a small pure-Python colour index
built on np_scores / int_scores of tests/color_search_cases.py.

colour_case() is also what tests/test_sort_similar_table.py feeds the device."""
import numpy as np
import pytest

import color_search_cases as CS
import test_sort_similar as TS
from cbird_amd import Media, SearchParams
from cbird_amd.database import sort_similar
from cbird_amd.index import Match
from sort_similar_table_rules import NO_MATCH, color_table, hamming_table, table_model


# ---- Hamming tables -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k, v in TS.VECTORS.items() if not v[2].get("max_thresh")])
def test_model_reproduces_the_hamming_vectors(name):
    hashes, ids, kw, (order, queries, not_found, behind) = TS.VECTORS[name]
    kw = dict(kw)
    got = table_model(hamming_table(hashes, kw.pop("thresh")), ids, **kw)
    assert got[:3] == (order, queries, not_found) and (behind is None or got[3] == behind)


@pytest.mark.parametrize("kw", [dict(), dict(min_matches=0), dict(min_matches=2, max_matches=2), dict(min_matches=3),
                                dict(min_matches=2, max_matches=1), dict(max_matches=1), dict(filter_parent=True),
                                dict(path_mode=1), dict(path_mode=2, max_matches=2), dict(look_behind=1),
                                dict(look_behind=8), dict(in_index=True), dict(hash0=True)])
def test_model_equals_the_hamming_model(kw):
    kw = dict(kw)
    h, ids, dir_id, under, _ = TS._rule_case(seed=11, n=60)
    in_index = None
    if kw.pop("in_index", False):
        in_index = np.ones(len(h), np.uint8)
        in_index[[0, 3, 4, 11, 30]] = 0
    if kw.pop("hash0", False):
        h[7] = 0
    want = TS.model(h, ids, 7, in_index=in_index, dir_id=dir_id, under=under, **kw)
    assert table_model(hamming_table(h, 7), ids, in_index=in_index, dir_id=dir_id, under=under, **kw) == want
    assert len(want[0]) > 1 or kw.get("min_matches", 1) > kw.get("max_matches", 5)


# ---- the colour index in numpy ------------------------------------------------------------------------------------------
class TinyColorIndex:
    """find / slice / find_index_data of ColorDescIndex (src/colordescindex.cpp:231-278) on the host"""

    def __init__(self, descs, ids, _rows=None):
        self.d, self.i = np.asarray(descs, CS.COLOR_DTYPE), np.asarray(ids, np.int64)
        self._rows = {} if _rows is None else _rows  # needle bytes -> {entry bytes: score}: slices share it

    def find_index_data(self, m):
        for k in np.flatnonzero(self.i == m.id)[:1]:
            m.colorDescriptor = self.d[k]
            return True
        return False

    def find(self, m, p=None):
        target = getattr(m, "colorDescriptor", None)
        if target is None or int(np.asarray(target, CS.COLOR_DTYPE)["numColors"]) <= 0:
            if not self.find_index_data(m):
                return []
            target = m.colorDescriptor
            if int(target["numColors"]) <= 0:
                return []
        if not len(self.i):
            return []
        s = CS.int_scores(CS.np_scores(np.asarray(target, CS.COLOR_DTYPE).reshape(1), self.d))[0]
        return [Match(int(self.i[k]), int(s[k])) for k in np.flatnonzero((s >= 0) & (self.i != 0))]

    def slice(self, media_ids):
        keep = np.isin(self.i, np.array(sorted(set(int(x) for x in media_ids)), np.int64))
        return TinyColorIndex(self.d[keep], self.i[keep], self._rows)


def colour_case(n, seed):
    """a selection and the index behind it: (media descriptors, ids in selection order, index descriptors, index ids)
    with ids shuffled, the index in an order of its own, 6 % of the items absent from the index, 6 % removed from it
    (id 0, descriptor cleared), 10 % of the Media carrying a descriptor that is not the index's, 10 % carrying none"""
    descs, _ = CS.synth_descriptors(n, seed)
    # the selection starts at the item with the most partners, so that there is a chain to follow
    start = int((CS.int_scores(CS.np_scores(descs, descs)) >= 0).sum(1).argmax())
    descs[[0, start]] = descs[[start, 0]]
    rng = np.random.default_rng([seed, n])
    ids = (rng.permutation(n) + 1).astype(np.uint32)
    kind = rng.random(n)
    kind[0] = 1.0  # the start is a plain item
    absent, gone = kind < 0.06, (kind >= 0.06) & (kind < 0.12)
    media = descs.copy()
    other = (kind >= 0.12) & (kind < 0.22)
    media[other] = descs[(np.flatnonzero(other) * 7 + 3) % n]
    media[(kind >= 0.22) & (kind < 0.32)] = np.zeros((), CS.COLOR_DTYPE)
    order = rng.permutation(np.flatnonzero(~absent))
    idx_d, idx_i = CS.removed(descs[order], ids[order], ids[gone])
    return media, ids, idx_d, idx_i


def colour_tables(media, ids, idx_d, idx_i):
    """(table uint16 [n, n] in selection order, in_index): what the loop's queries see"""
    n = len(ids)
    where = {int(i): k for k, i in enumerate(idx_i) if i}
    in_index = np.array([int(i) in where for i in ids], np.uint8)
    entry = np.zeros(n, CS.COLOR_DTYPE)
    for k, i in enumerate(ids):
        if in_index[k]:
            entry[k] = idx_d[where[int(i)]]
    needle = entry.copy()
    needle[media["numColors"] > 0] = media[media["numColors"] > 0]
    return color_table(needle, entry, CS.np_scores, CS.int_scores), in_index


def media_of(descs, ids, paths=None):
    out = []
    for k, (d, i) in enumerate(zip(descs, ids)):
        m = Media(id=int(i), path=paths[k] if paths else f"/db/{int(i)}.jpg")
        m.colorDescriptor = d.copy()
        out.append(m)
    return out


def colour_params(**kw):
    return SearchParams(algo=SearchParams.AlgoColor, **kw)


def test_the_fixture_has_what_a_wrong_table_would_trip_over():
    d, ids = CS.synth_descriptors(96, 5)
    t = color_table(d, d, CS.np_scores, CS.int_scores).astype(np.int64)
    n = len(d)
    off = ~np.eye(n, dtype=bool)
    finite = (t != NO_MATCH) & off
    assert 0.10 < finite.sum() / off.sum() < 0.20                # most pairs do not match: chains break off
    asym = np.triu(finite & finite.T & (t != t.T), 1)
    assert asym.sum() >= 1                                       # int(d(a, b)) != int(d(b, a)): a transposed table shows
    print("finite %.3f asymmetric pairs %d lonely %d colourless %d" % (
        finite.sum() / off.sum(), asym.sum(), (~finite.any(1)).sum(), (d["numColors"] == 0).sum()))
    assert (~finite.any(1)).sum() >= 1                           # items with no partner at all
    assert (d["numColors"] == 0).sum() >= 1                      # descriptors without colours: FLT_MAX rows and columns
    assert (finite.sum() / off.sum()).round(2) == 0.14 and asym.sum() == 116 and (~finite.any(1)).sum() == 10


@pytest.mark.parametrize("kw", [dict(), dict(minMatches=0), dict(minMatches=2), dict(minMatches=2, maxMatches=2),
                                dict(maxMatches=1), dict(filterParent=True), dict(path="in", inPath=True),
                                dict(path="in", inPath=False, maxMatches=2)])
def test_model_equals_the_loop_on_a_colour_index(kw):
    media, ids, idx_d, idx_i = colour_case(96, 5)
    n = len(ids)
    rng = np.random.default_rng(3)
    dirs, under = rng.integers(0, 3, n), rng.integers(0, 2, n).astype(np.uint8)
    paths = [f"/db/{'in' if under[k] else 'out'}/d{dirs[k]}/{int(ids[k])}.jpg" for k in range(n)]
    dir_id = (dirs + 3 * under).astype(np.uint32)
    table, in_index = colour_tables(media, ids, idx_d, idx_i)
    assert in_index.sum() < n and (media["numColors"] == 0).any() and (idx_i == 0).any()
    p = colour_params(**kw)
    got, q, nf = sort_similar(TinyColorIndex(idx_d, idx_i), media_of(media, ids, paths), p, batched=False, db_path="/db")
    mode = 0 if p.path == "" else (1 if p.inPath else 2)
    want = table_model(table, ids, p.minMatches, p.maxMatches, in_index, dir_id, under, p.filterParent, mode)
    assert ([m.id for m in got], q, nf) == want[:3]
    if not kw:
        assert len(want[0]) > 3 and want[3] > 0  # a chain with look-behind inserts, not a degenerate case
        # the transposed table is another chain: the asymmetric pairs decide somewhere
        assert table_model(table.T, ids, in_index=in_index)[:3] != want[:3]
