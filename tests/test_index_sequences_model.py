"""The host side of tests/test_index_sequences.py, checked without a device: the mirrors of tests/index_sequences.py
against a second, naive recomputation (filter and append on plain Python lists) and against brute force over the
definitions, and the coverage conditions every (kind, seed) of the device tests has to meet -- conditions, asserted, so
that a weak seed cannot hide a gap."""
import numpy as np
import pytest

import index_sequences as S
import index_sequences_cv as V
import index_sequences_video as W
import test_index_sequences as T

ALL = [(kind, name) for kind in S.KINDS for name, _ in T.cases(kind)]
ALL_CV = [(kind, name) for kind in V.KINDS for name, _ in T.cases(kind)]


def _ops(kind, name):
    return dict(T.cases(kind))[name]


class Naive:
    """a handle as a list of [hash, id] rows"""

    def __init__(self, zero_hash, rows=()):
        self.zero_hash, self.rows = zero_hash, [list(r) for r in rows]

    def apply(self, op, a):
        if op[0] == "load":
            self.rows = [[int(h), int(i)] for h, i in zip(a["h"], a["ids"])]
        elif op[0] == "add":
            self.rows += [[int(h), int(i)] for h, i in zip(a["h"], a["ids"])]
        elif op[0] == "remove":
            gone = set(int(x) for x in a["ids"])
            self.rows = [[0 if self.zero_hash and i in gone else h, 0 if i in gone else i] for h, i in self.rows]
        elif op[0] == "slice":
            want = set(int(x) for x in a["ids"])
            return Naive(self.zero_hash, [r for r in self.rows if r[1] in want])
        return None


def _popcount(x):
    return bin(x).count("1")


def _brute_find(rows, q, thresh):
    """DctHashIndex::find from its definition: live entries closer than thresh, in (score, id) order"""
    if q == 0:
        return []
    return sorted(((i, _popcount(h ^ q)) for h, i in rows if i != 0 and _popcount(h ^ q) < thresh), key=lambda r: (r[1], r[0]))


@pytest.mark.parametrize("name", sorted(n for n in S.HAND if not n.startswith("color")))
def test_the_mirror_equals_a_naive_recomputation_after_every_step(orc, name):
    """contents after every step of the hand-written sequences; removal keeps count() and zeroes the id (and, for a
    DctHashIndex, the hash); a slice is the parent's rows with a wanted id, in order; ids are never handed out twice"""
    kind = "dcthash" if name.startswith("dcthash") else name
    world = S.World(kind)
    naive = [Naive(kind == "dcthash")]
    searched = 0
    for op in S.HAND[name]:
        a = S.resolve(world, op)
        if S.is_search(op):
            m, nv = world.handles[op[1]], naive[op[1]]
            want = S.canon(S.expect(world, op, a, orc))
            if kind == "dcthash" and op[0] == "find_batch" and searched < 6:  # the oracle's answer against the definition
                searched += 1
                wi, ws, wc = want
                for j, q in enumerate(a["q"].tolist()[:16]):
                    brute = _brute_find(nv.rows, q, op[4])
                    assert wc[j] == len(brute), (op, j)
                    assert list(zip(wi[j], ws[j]))[:len(brute)] == [tuple(r) for r in brute[:op[5]]], (op, j)
            if op[0] == "download":
                assert want == [[r[0] for r in nv.rows], [r[1] for r in nv.rows]]
            if op[0] == "hashes_for_id":
                assert want == [r[0] for r in nv.rows if r[1] == a["id"]]
            continue
        before = world.handles[op[1]].count()
        sl = naive[op[1]].apply(op, a)
        S.apply_mutation(world, op, a)
        if sl is not None:
            naive.append(sl)
        if op[0] in ("remove", "add_refused"):
            assert world.handles[op[1]].count() == before
        for m, nv in zip(world.handles, naive):
            assert m.h.tolist() == [r[0] for r in nv.rows] and m.ids.tolist() == [r[1] for r in nv.rows], op
        if kind == "dcthash":
            live = world.handles[op[1]].ids
            live = live[live != 0]
            assert len(np.unique(live)) == len(live), op
    assert len(world.handles) == len(naive) >= 2 or name == "dcthash_tree"


def test_the_masked_search_of_the_mirror_is_the_leaf_of_the_needle(orc):
    """hand sequence "dcthash_tree": before the remove every needle sees the entries that share its bit 0; after it the
    needles with bit 0 clear see the ones that share bits 0 and 1 (8300 values, the zeroed ones among them, under prefix 0)"""
    world = S.World("dcthash")
    masks = []
    for op in S.HAND["dcthash_tree"]:
        a = S.resolve(world, op)
        if op[0] == "tree_masks":
            masks.append((a["q"], S.expect(world, op, a, orc)))
        elif not S.is_search(op):
            S.apply_mutation(world, op, a)
    (_, before), (q, after) = masks  # (the needles are drawn from the contents: each step has its own)
    assert (before == 1).all()
    even = (q & np.uint64(1)) == 0
    assert even.any() and (~even).any()
    assert (after[even] == 3).all() and (after[~even] == 1).all()


@pytest.mark.parametrize("kind,name", ALL)
def test_the_seeds_in_use_meet_every_condition(kind, name):
    ops = _ops(kind, name)
    f = S.coverage(kind, ops)
    assert f["max_needles"] <= 64
    if name == "hand_dcthash_tree":  # one boundary: the tree's shape under remove()
        assert f["tree_kinds"] == {"internal"} and f["max_slots"] == 16000
        return
    if name == "hand_color_refused_add_leaves_nothing_behind":  # one thing: an add after a refused add, then searches
        assert f["refused_then_add"]
        return
    assert f["ops"] >= 40
    routes = set(S.ROUTES[kind])
    if kind == "color":
        # from 4000 entries across 4096, and across the next growth
        assert f["crossings0"] == [0, 4096, 10240], f["crossings0"]
        assert f["route_after_mutation"] >= routes and f["route_second_in_row"] >= routes
        assert f["mutation_then_search"] >= set(S.COLOR_MUTATIONS), set(S.COLOR_MUTATIONS) - f["mutation_then_search"]
        assert f["slice_parent_used"] and f["slice_itself_used"] and f["remove_all_then_add"]
        # 3 of 7 and 128 of 255 kept (planes with one entry of slack, and with none), each added to afterwards
        assert f["slices_added_to"] >= {(7, 3), (255, 128)}, f["slices_added_to"]
        # an add after a refused add, then a search
        assert f["refused_then_add"]
        return
    # capacity: 1024 is crossed, and two later steps of the growth by half
    grown = [c for c in f["crossings0"] if c]
    assert 1024 in grown and len(grown) >= 3, f["crossings0"]
    # placement of the searches
    assert f["route_after_mutation"] >= routes, routes - f["route_after_mutation"]
    assert f["route_second_in_row"] >= routes, routes - f["route_second_in_row"]
    assert f["mutation_then_search"] >= set(S.MUTATIONS), set(S.MUTATIONS) - f["mutation_then_search"]
    assert f["slice_parent_used"] and f["slice_itself_used"] and f["remove_all_then_add"]
    # a block of 1024 records and a result that does not fit it
    # ... where the block is known to be that small (index_sequences.RescanRule): on a plain handle, on five shards
    assert f["rescans"] >= 1 and f["rescans_shards5"] >= 1
    if kind == "dcthash":  # ... and on the handle of the start, after cluster_labels has given its block back
        assert f["rescans_parent"] >= 1
    # the three join kernels, and a search after a remove (the mutation that keeps a stale table's size right)
    assert f["join_thresholds"] == set(S.JOIN_THRESHOLDS) and f["stale_join_chances"] >= 1
    if name.startswith("hand_fdct"):
        assert f["tree_kinds"] == {"leaf", "internal"} and 8192 in f["crossings0"]


def test_the_generator_is_deterministic():
    for kind in S.KINDS:
        assert S.sequence(kind, 5) == S.sequence(kind, 5) != S.sequence(kind, 6)
        assert eval(repr(S.sequence(kind, 5))) == S.sequence(kind, 5)  # (a printed sequence can be pasted back)


def test_the_colour_mirror_equals_a_naive_recomputation_after_every_step(orc):
    """hand sequence "color": entries as a plain list of (id, descriptor bytes); removal clears both in place, a slice keeps
    the wanted ids in order, a refused add changes nothing; find() of the mirror is np_scores' int() in index order"""
    import color_search_cases as CS

    world, naive = S.World("color"), [[]]
    checked = 0
    for op in S.HAND["color"]:
        a = S.resolve(world, op)
        m, nv = world.handles[op[1]], naive[op[1]]
        if S.is_search(op):
            want = S.canon(S.expect(world, op, a, orc))
            if op[0] == "download":
                assert want == [[i for i, _ in nv], b"".join(d for _, d in nv)]
            if op[0] == "find" and checked < 3:
                checked += 1
                sc = CS.int_scores(CS.np_scores(np.array([a["d"]]), m.d))[0]
                assert want == [[i, int(x)] for (i, _), x in zip(nv, sc) if i and x >= 0]
            continue
        if op[0] == "add":
            nv += [(int(i), d.tobytes()) for i, d in zip(a["ids"], a["d"])]
        elif op[0] == "remove":
            gone = set(int(x) for x in a["ids"]) - {0}
            nv[:] = [(0, bytes(258)) if i in gone else (i, d) for i, d in nv]
        elif op[0] == "slice":
            want = set(int(x) for x in a["ids"])
            naive.append([(i, d) for i, d in nv if i in want])
        S.apply_mutation(world, op, a)
        for mm, rows in zip(world.handles, naive):
            assert mm.ids.tolist() == [i for i, _ in rows] and mm.d.tobytes() == b"".join(d for _, d in rows), op
    assert len(naive) == 5


@pytest.mark.parametrize("kind,name", ALL_CV)
def test_the_256_bit_seeds_in_use_meet_every_condition(kind, name):
    f = V.coverage(kind, _ops(kind, name))
    routes = set(V.ROUTES)
    assert f["ops"] >= 40 and f["max_needles"] <= 32
    assert f["route_after_mutation"] >= routes, routes - f["route_after_mutation"]
    assert f["route_second_in_row"] >= routes, routes - f["route_second_in_row"]
    assert f["slice_parent_used"] and f["slice_itself_used"] and f["remove_all_then_add"]
    if kind == "cv":
        assert f["mutation_then_search"] >= set(V.MUTATIONS)
        assert f["crossings0"] == [0, 65536] and f["refused_then_add"]  # 65 000 rows, then across 65 536
    else:
        assert f["mutation_then_search"] >= set(V.MUTATIONS) - {"add_refused"}
        # every shard has been the current one twice, and a search followed each change of shard but the first
        assert min(f["turns0"]) >= 2 and f["searches_between_runs"] >= 4, (f["turns0"], f["searches_between_runs"])


@pytest.mark.parametrize("kind", V.KINDS)
def test_the_256_bit_mirror_equals_a_naive_recomputation_after_every_step(kind):
    """hand sequences: the matrix as a list of (media id, row bytes) per row; removal renames a media's rows to id 0 and
    keeps them; a slice is the wanted media in ascending id; knn of the mirror against brute force on the first searches"""
    from oracle import CvOracle

    cvo = CvOracle()
    world, naive, checked = V.World(kind), [[]], 0
    for op in V.HAND[kind]:
        a = V.resolve(world, op)
        m, nv = world.handles[op[1]], naive[op[1]]
        if V.is_search(op):
            want = S.canon(V.expect(world, op, a, cvo))
            if op[0] == "descriptors":
                rows = [r for i, r, orig in nv if orig == a["id"]]
                assert want == [list(r) for r in rows]
            if op[0] == "knn" and checked < 2:
                checked += 1
                bits = np.unpackbits(m.rows, axis=1)
                for q in range(0, len(a["q"]), 8):
                    dist = (bits != np.unpackbits(a["q"][q])).sum(1)
                    order = np.lexsort((np.arange(len(dist)), dist))
                    order = order[dist[order] < op[5]]
                    assert want[q] == [len(order), order[:op[4]].tolist(), dist[order[:op[4]]].tolist()]
            continue
        if op[0] == "add":
            for mid, rows in zip(a["ids"].tolist(), a["rows"]):
                nv += [(mid, bytes(r), mid) for r in rows]
        elif op[0] == "remove":
            gone = set(int(x) for x in a["ids"])
            nv[:] = [(0 if i in gone else i, r, orig) for i, r, orig in nv]
        elif op[0] == "slice":
            want = sorted(set(int(x) for x in a["ids"]))
            naive.append([(i, r, orig) for w in want for i, r, orig in nv if i == w])
        V.apply_mutation(world, op, a)
        for mm, rows in zip(world.handles, naive):
            assert mm.rows.tobytes() == b"".join(r for _, r, _ in rows), op
            assert mm.media_of_rows(np.arange(mm.count())).tolist() == [i for i, _, _ in rows], op


@pytest.mark.parametrize("name", [n for n, _ in T.cases("video")])
def test_the_video_seeds_in_use_meet_every_condition(name):
    f = W.coverage(_ops("video", name))
    routes = set(W.ROUTES)
    assert f["ops"] >= 40 and f["max_needles"] <= 64
    assert f["route_after_mutation"] >= routes, routes - f["route_after_mutation"]
    assert f["route_second_in_row"] >= routes, routes - f["route_second_in_row"]
    assert f["mutation_then_search"] >= set(W.MUTATIONS), set(W.MUTATIONS) - f["mutation_then_search"]
    assert f["slice_parent_used"] and f["slice_itself_used"] and f["remove_all_then_add"]
    assert f["skips"] == set(W.SKIPS)
    # another skipFrames without a mutation in between (must not rebuild), and with one (must rebuild)
    assert f["skip_change_without_rebuild"] >= 1 and f["skip_change_with_rebuild"] >= 1
    assert f["frames_batch_first_after_mutation"] >= 1
    # a media id held twice, a clip without a usable hash, a clip with lastFrame / 2 <= skip, all while searched
    assert f["doubled_id"] and f["dull"] and f["short_clip_untrimmed"]
    # coverage and segments: pairs under both skips, and pairs that name an id held twice, the all-dull clip, a removed id
    for route in ("coverage", "segments"):
        have = f["pairs"][route]
        assert {s for k, s in have if k == "pair"} == set(W.SKIPS), (route, have)
        assert {k for k, _ in have} >= {"pair", "doubled", "dull", "removed"}, (route, have)


def test_the_video_mirror_builds_when_the_reference_does():
    """hand sequence: the videos against a naive list; the built skip against the rule "the first search after a mutation
    builds with its own skipFrames, nothing else does" restated on the op list alone"""
    from oracle import VideoOracle

    vorc = VideoOracle()
    world, naive = W.World(), [[]]
    dirty, built_skip = {0: True}, {}
    for op in W.HAND:
        a = W.resolve(world, op)
        t = op[1]
        if W.is_search(op):
            if not (op[0] == "find_frame" and a["needle"][0] == 0) and op[0] not in ("coverage", "segments"):
                if dirty[t]:
                    dirty[t], built_skip[t] = False, op[-1]
            want, entries = W.expect(world, op, a, vorc, 0)
            if entries is not None:
                assert world.handles[t].built_skip == built_skip[t], op
                assert entries == len(vorc.build_entries(world.handles[t].videos, built_skip[t])[0])
            continue
        if op[0] == "slice":
            want = [int(x) for x in a["ids"]]
            held = [v[0] for v in naive[t]]
            naive.append([naive[t][held.index(i)] for i in dict.fromkeys(want) if i in held])
            dirty[len(naive) - 1] = True
        elif op[0] == "remove":
            gone = set(int(x) for x in a["ids"])
            naive[t] = [v for v in naive[t] if v[0] not in gone]
            dirty[t] = True
        else:
            naive[t] = naive[t] + [(int(i), f.tolist(), h.tolist()) for i, (f, h) in zip(a["ids"], a["clips"])]
            dirty[t] = True
        W.apply_mutation(world, op, a)
        for m, rows in zip(world.handles, naive):
            assert [(v[0], v[1].tolist() if hasattr(v[1], "tolist") else v[1]) for v in m.videos] == [(v[0], v[1]) for v in rows], op
