"""Random and hand-written sequences of mutations and searches on the long-lived index handles that hold two columns --
the 64-bit ones (DctHashIndex, DctFeaturesIndex) and the colour index -- with a host
mirror that says what every search must answer.  Pure Python and NumPy: nothing here touches a device.

A sequence is a list of ops.  An op is a tuple of a name and plain ints / tuples (`repr` of a list of ops can be pasted
back as a hand-written sequence); everything an op needs beyond that -- hashes, ids, needles -- is drawn from
np.random.default_rng of the seeds the op carries and from the mirror's contents at that step (resolve()).  The first
argument of every op is the number of the handle it works on: 0 is the handle the sequence starts with, every `slice`
appends one.

Kinds:
  "dcthash"    DctHashIndex: one id per slot; remove zeroes the id AND the hash (cbh_idx64_remove)
  "fdct"       DctFeaturesIndex, exact candidates: an id per image with several hashes; remove zeroes ids only
  "fdct_tree"  DctFeaturesIndex(tree_compat=True): as "fdct" with the HammingTree's candidate sets
  "color"      ColorDescIndex: an id and a 258-byte descriptor per entry; remove zeroes the id and clears the descriptor
               (color_search_cases.removed); scores are color_search_cases.np_scores, bit for bit

The semantics are the ones the existing tests state, not new ones: removal as tests/test_slice_device.py::_build64 and
tests/test_join_resident.py (id 0, hash 0 for a DctHashIndex, id 0 alone for a DctFeaturesIndex; count() unchanged),
slice as np.isin on the parent's ids (test_idx64_slice_equals_isin_on_the_parent), load on a loaded handle as a reload
(tests/test_join_resident.py::_reload), searchIndex as cbird_amd/database.py::search_index.

Ops (t = handle number):
  mutations  ("load", t, n, seed, ones)  dcthash: n slots; ones != None: exactly the first `ones` hashes have bit 0 set
             ("load", t, m, k, seed)     fdct: m images of k hashes
             ("add", t, n, seed) / ("add", t, m, k, seed)
             ("add_refused", t)          an add with the next allocation refused: CBH_E_NOMEM, nothing changes (plain
                                         handles; a sharded handle leaves it out)
             ("remove", t, spec)         spec: ("all",) | ("ids", (..)) | ("range", lo, hi) | ("draw", seed, count): ids
                                         that are live, already removed, absent, and repeated
             ("slice", t, seed, num, den)  keeps num/den of the live ids (and asks for an absent one); the slice becomes
                                         handle number len(handles)
             ("set_record_capacity", t, records), ("join_prepare", t, thresh), ("join_release", t)
  searches   dcthash: ("find", t, seed, thresh), ("find_batch", t, seed, nq, thresh, k),
             ("find_masked", t, seed, nq, thresh, k), ("search_index_batch", t, seed, nq, thresh, max_thresh,
             min_matches, max_matches), ("find_coalesced", t, seed, nq, thresh), ("cluster_labels", t, thresh),
             ("download", t), ("tree_masks", t, seed, nq)
             fdct: ("find", t, seed, thresh), ("find_by_id", t, seed, thresh), ("find_batch", t, seed, nn, thresh),
             ("hashes_for_id", t, seed), ("tree_masks", t, seed, nq), ("download", t)
  color      mutations: ("add", t, n, seed), ("add_refused", t), ("remove", t, spec), ("slice", t, seed, num, den) with
             den == 0: exactly num of the live ids;  searches: ("find", t, seed), ("find_by_id", t, seed),
             ("find_batch", t, seed, nq, k), ("distances", t, seed, nq), ("sort_similar", t, seed, n), ("download", t)
"""
import numpy as np

KINDS = ("dcthash", "fdct", "fdct_tree", "color")
MUTATIONS = ("load", "add", "add_refused", "remove", "slice", "set_record_capacity", "join_prepare", "join_release")
# what changes the contents (the others change how the next search is run)
CONTENT_MUTATIONS = ("load", "add", "remove")
ROUTES = {
    "dcthash": ("find", "find_batch", "find_batch65", "find_masked", "search_index_batch", "find_coalesced",
                "cluster_labels", "download"),
    "fdct": ("find", "find_by_id", "find_batch", "hashes_for_id", "tree_masks", "download"),
}
ROUTES["fdct_tree"] = ROUTES["fdct"]
ROUTES["color"] = ("find", "find_by_id", "find_batch", "distances", "sort_similar", "download")
COLOR_MUTATIONS = ("add", "add_refused", "remove", "slice")
REC_CAP_DEFAULT = 1 << 24  # cbh_idx64::rec_cap_default
SMALL_REC_CAP = 1024
JOIN_THRESHOLDS = (4, 5, 8)  # the three join kernels, two plan sizes (m = max(4, thresh))
TREE_LEAF = 8192  # fdct.hip: a node is internal iff more than 8192 values share its prefix

_NBASES = 48
_BASES = np.random.default_rng(20241).integers(1 << 8, 1 << 63, _NBASES, dtype=np.uint64)


def gen_hashes(seed, n, ones=None):
    """n non-zero hashes, each one of 48 base values with up to three bits flipped: a needle drawn from one of them is
    within distance 6 of about n / 48 others.  ones: the first `ones` hashes get bit 0 set, the others cleared."""
    rng = np.random.default_rng([int(seed), int(n), 7])
    h = _BASES[rng.integers(0, _NBASES, n)].copy()
    for _ in range(3):
        bit = np.uint64(1) << rng.integers(1, 64, n).astype(np.uint64)
        h ^= np.where(rng.random(n) < 0.5, bit, np.uint64(0))
    if ones is not None:
        h = (h & ~np.uint64(1)) | (np.arange(n) < ones).astype(np.uint64)
    assert (h != 0).all()
    return h


def grow_capacity(cap, need):
    """cbh_idx64::reserve: by half, in 1024-row chunks"""
    if need <= cap:
        return cap
    return (max(need, cap + cap // 2) + 1023) // 1024 * 1024


def is_search(op):
    return op[0] not in MUTATIONS


def route_of(op):
    """the name a search op has in ROUTES (find_batch with k > 64 is the sort path: a route of its own)"""
    if op[0] == "find_batch" and len(op) == 6 and op[5] > 64:
        return "find_batch65"
    return op[0]


class Mirror64:
    """what a cbh_idx64 holds: two columns, in slot order"""

    def __init__(self, zero_hash):
        self.zero_hash = zero_hash
        self.h = np.zeros(0, np.uint64)
        self.ids = np.zeros(0, np.uint32)
        self.cap = 0  # the plain handle's capacity (a sharded handle's shards have their own)
        self.crossings = []  # capacities left behind by add / load
        self.rec_cap = REC_CAP_DEFAULT
        self.opted = False

    def count(self):
        return len(self.h)

    def _reserve(self, need):
        ncap = grow_capacity(self.cap, need)
        if ncap != self.cap:
            self.crossings.append(self.cap)
            self.cap = ncap

    def load(self, h, ids):
        self.h, self.ids = np.array(h, np.uint64), np.array(ids, np.uint32)
        self._reserve(len(self.h))

    def add(self, h, ids):
        self.h = np.concatenate([self.h, np.asarray(h, np.uint64)])
        self.ids = np.concatenate([self.ids, np.asarray(ids, np.uint32)])
        self._reserve(len(self.h))

    def remove(self, ids):
        gone = np.isin(self.ids, np.asarray(ids, np.uint32))
        self.ids = np.where(gone, np.uint32(0), self.ids)
        if self.zero_hash:
            self.h = np.where(gone, np.uint64(0), self.h)

    def slice(self, ids):
        keep = np.isin(self.ids, np.asarray(ids, np.uint32))
        out = Mirror64(self.zero_hash)
        out.load(self.h[keep], self.ids[keep])
        return out

    def live_ids(self):
        return np.unique(self.ids[self.ids != 0])


def grow_capacity_color(cap, need):
    """color.hip grow_index: by half and 4096, even"""
    if need <= cap:
        return cap
    return (max(need, cap + cap // 2 + 4096) + 1) & ~1


class MirrorColor:
    """what a cbh_color holds: ids and descriptors in add order"""

    def __init__(self, d=None, ids=None, cap=0):
        import color_search_cases as CS

        self.d = np.zeros(0, CS.COLOR_DTYPE) if d is None else d
        self.ids = np.zeros(0, np.uint32) if ids is None else ids
        self.cap = cap  # (a slice: the kept entries rounded up to 4)
        self.crossings = []

    def count(self):
        return len(self.ids)

    def add(self, d, ids):
        self.d, self.ids = np.concatenate([self.d, d]), np.concatenate([self.ids, np.asarray(ids, np.uint32)])
        ncap = grow_capacity_color(self.cap, len(self.ids))
        if ncap != self.cap:
            self.crossings.append(self.cap)
            self.cap = ncap

    def remove(self, ids):
        import color_search_cases as CS

        self.d, self.ids = CS.removed(self.d, self.ids, ids)

    def slice(self, ids):
        keep = np.isin(self.ids, np.asarray(ids, np.uint32))
        return MirrorColor(self.d[keep].copy(), self.ids[keep].copy(), (int(keep.sum()) + 3) & ~3)

    def live_ids(self):
        return np.unique(self.ids[self.ids != 0])


class World:
    """the handles of one sequence and the ids it has handed out"""

    def __init__(self, kind):
        assert kind in KINDS, kind
        self.kind = kind
        self.handles = [MirrorColor() if kind == "color" else Mirror64(zero_hash=kind == "dcthash")]
        self.next_id = 1

    def take_ids(self, n):
        first = self.next_id
        self.next_id += n
        return np.arange(first, first + n, dtype=np.uint32)


# ---- from an op to the arrays it stands for ---------------------------------------------------------------------------
def _rows(world, op):
    """(hashes, ids) of a load / add"""
    if world.kind == "dcthash":
        n, seed = op[2], op[3]
        ones = op[4] if op[0] == "load" and len(op) > 4 else None
        return gen_hashes(seed, n, ones), world.take_ids(n)
    m, k, seed = op[2], op[3], op[4]
    return gen_hashes(seed, m * k), np.repeat(world.take_ids(m), k)


def _remove_ids(world, m, spec):
    if spec[0] == "all":
        return m.live_ids()
    if spec[0] == "ids":
        return np.array(spec[1], np.uint32)
    if spec[0] == "range":
        return np.arange(spec[1], spec[2], dtype=np.uint32)
    assert spec[0] == "draw", spec
    rng = np.random.default_rng([spec[1], 11])
    live, ever = m.live_ids(), np.arange(1, max(world.next_id, 2), dtype=np.uint32)
    some = rng.choice(live, min(spec[2], len(live)), replace=False) if len(live) else live
    gone = np.setdiff1d(ever, live)[:3]  # removed earlier, or never in this handle
    absent = np.array([world.next_id + 5, 0xfffffff0], np.uint32)
    return np.concatenate([some, some[:2], gone, absent]).astype(np.uint32)  # (some[:2]: repeated)


def _slice_ids(world, m, op):
    rng = np.random.default_rng([op[2], 13])
    live = m.live_ids()
    want = len(live) * op[3] // op[4]
    some = np.sort(rng.choice(live, want, replace=False)) if want else live[:0]
    return np.concatenate([some, [world.next_id + 9]]).astype(np.uint32)


def _needles64(m, seed, nq):
    """nq needle hashes: entries of the index with 0..2 bits flipped, fresh values of the same bases, a few strangers
    and one 0"""
    rng = np.random.default_rng([seed, 17])
    fresh = gen_hashes(seed + 1000003, nq)
    q = fresh.copy()
    live = np.flatnonzero((m.ids != 0) & (m.h != 0))
    if len(live):
        take = rng.random(nq) < 0.6
        q[take] = m.h[rng.choice(live, int(take.sum()))]
    for _ in range(2):
        bit = np.uint64(1) << rng.integers(0, 64, nq).astype(np.uint64)
        q ^= np.where(rng.random(nq) < 0.4, bit, np.uint64(0))
    strangers = rng.random(nq) < 0.1
    q[strangers] = rng.integers(1, 1 << 63, int(strangers.sum()), dtype=np.uint64)
    if nq > 2:
        q[int(rng.integers(0, nq))] = 0
    return q


def _needle_images(m, seed, nn):
    """nn needle images of a DctFeaturesIndex: (id, hashes) -- the hashes of an indexed image, some flipped, some replaced,
    one 0; every third needle is a stranger with id 0"""
    rng = np.random.default_rng([seed, 19])
    live = m.live_ids()
    out = []
    for j in range(nn):
        if len(live) and j % 3 != 2:
            mid = int(rng.choice(live))
            kp = m.h[m.ids == mid][:40].copy()
        else:
            mid, kp = 0, gen_hashes(seed + 31 * j, int(rng.integers(1, 30)))
        kp[::4] ^= np.uint64(1) << np.uint64(int(rng.integers(0, 64)))
        if len(kp) > 5:
            kp[5] = 0
        out.append((mid, kp))
    return out


def resolve(world, op):
    """the arguments of the real call: a dict; mutates nothing but world.next_id (ids handed out)"""
    name, m = op[0], world.handles[op[1]]
    if world.kind == "color":
        return _resolve_color(world, op, m)
    fd = world.kind != "dcthash"
    if name in ("load", "add"):
        h, ids = _rows(world, op)
        return {"h": h, "ids": ids}
    if name == "add_refused":
        n = m.count() // 2 + 2048  # past any capacity the growth rule can have left behind
        return {"h": gen_hashes(4242, n), "ids": np.arange(1, n + 1, dtype=np.uint32) + np.uint32(1 << 30)}
    if name == "remove":
        return {"ids": _remove_ids(world, m, op[2])}
    if name == "slice":
        return {"ids": _slice_ids(world, m, op)}
    if name in ("find_batch", "find_masked", "search_index_batch", "find_coalesced", "tree_masks") and not (fd and name == "find_batch"):
        q = _needles64(m, op[2], op[3])
        if name == "search_index_batch":  # needle ids: the entry a needle equals, if any (filterSelf has something to do)
            pos = {int(x): int(i) for x, i in zip(m.h.tolist(), m.ids.tolist()) if x and i}
            return {"q": q, "nid": np.array([pos.get(int(x), 0) for x in q], np.uint32)}
        if name == "find_coalesced":
            q = q[q != 0]
        return {"q": q}
    if name == "find" and not fd:
        q = _needles64(m, op[2], 4)
        return {"q": int(q[q != 0][0])}
    if name == "find" and fd:
        mid, kp = _needle_images(m, op[2], 2)[op[2] % 2]
        return {"id": mid, "kp": kp}
    if name == "find_by_id":
        live = m.live_ids()
        rng = np.random.default_rng([op[2], 23])
        return {"id": int(rng.choice(live)) if len(live) else world.next_id + 3, "kp": np.zeros(0, np.uint64)}
    if name == "find_batch" and fd:
        return {"needles": _needle_images(m, op[2], op[3])}
    if name == "hashes_for_id":
        ever = np.arange(1, max(world.next_id, 2) + 1)
        return {"id": int(np.random.default_rng([op[2], 29]).choice(ever))}
    return {}


# ---- what the searches must answer ------------------------------------------------------------------------------------
def _pairs(ids, scores):
    return list(zip(np.asarray(ids).tolist(), np.asarray(scores).tolist()))


def _find_batch(orc, h, ids, q, thresh, k):
    if len(h) == 0:
        return np.zeros((len(q), k), np.uint32), np.zeros((len(q), k), np.int32), np.zeros(len(q), np.uint32)
    return orc.find64_batch(h, ids, q, thresh, k)


def masked_batch(orc, h, ids, q, masks, thresh, k):
    """find64_batch where needle j only sees the entries with ((q[j] ^ hash) & masks[j]) == 0"""
    oi, od, oc = np.zeros((len(q), k), np.uint32), np.zeros((len(q), k), np.int32), np.zeros(len(q), np.uint32)
    groups = {}
    for j, (x, mk) in enumerate(zip(q.tolist(), masks.tolist())):
        groups.setdefault((mk, x & mk), []).append(j)
    for (mk, low), js in groups.items():
        sel = (h & np.uint64(mk)) == np.uint64(low)
        if sel.any():
            oi[js], od[js], oc[js] = orc.find64_batch(h[sel], ids[sel], q[js], thresh, k)
    return oi, od, oc


def search_index(orc, h, ids, q, nid, thresh, max_thresh, min_matches, max_matches):
    """cbird_amd/database.py::search_index for one needle hash: escalation, filterSelf, the cut"""
    def find(t):
        return _pairs(*orc.find64(h, ids, q, t)) if q and len(h) else []

    t, found = thresh, find(thresh)
    if max_thresh > 0:
        while len(found) <= min_matches and t + 1 <= max_thresh:
            t += 1
            found = find(t)
    return [(i, s) for i, s in found if i != nid][:max_matches]


def expect(world, op, a, orc):
    """the answer of search `op` (arguments `a` from resolve) on the mirror: plain lists and arrays"""
    import clusters_rules

    name, m = op[0], world.handles[op[1]]
    if world.kind == "color":
        return _expect_color(op, a, m)
    h, ids = m.h, m.ids
    if world.kind == "dcthash":
        if name == "find":
            return _pairs(*orc.find64(h, ids, a["q"], op[3])) if len(h) else []
        if name == "find_batch":
            return _find_batch(orc, h, ids, a["q"], op[4], op[5])
        if name == "tree_masks":
            return orc.htree_leaf_masks(h, a["q"])
        if name == "find_masked":
            return masked_batch(orc, h, ids, a["q"], orc.htree_leaf_masks(h, a["q"]), op[4], op[5])
        if name == "search_index_batch":
            return [search_index(orc, h, ids, int(x), int(i), *op[4:8]) for x, i in zip(a["q"], a["nid"])]
        if name == "find_coalesced":
            return [_pairs(*orc.find64(h, ids, int(x), op[4])) if len(h) else [] for x in a["q"]]
        if name == "cluster_labels":
            return clusters_rules.cluster_labels(h, ids, op[2])
        if name == "download":
            return h, ids
        raise ValueError(op)
    tree = world.kind == "fdct_tree"

    def fdct(mid, kp, thresh):
        if len(kp) == 0 and mid > 0:
            kp = h[ids == mid]  # _tree->findIndex
        if len(kp) == 0 or len(h) == 0:
            return []
        f = orc.fdct_find_tree if tree else orc.fdct_find
        return _pairs(*f(h, ids, kp, mid, thresh))

    if name in ("find", "find_by_id"):
        return fdct(a["id"], a["kp"], op[3])
    if name == "find_batch":
        return [fdct(mid, kp, op[4]) for mid, kp in a["needles"]]
    if name == "hashes_for_id":
        return h[ids == a["id"]]
    if name == "tree_masks":
        return orc.htree_leaf_masks(h, a["q"])
    if name == "download":
        return h, ids
    raise ValueError(op)


# ---- the colour index -------------------------------------------------------------------------------------------------
def _color_needles(m, seed, nq):
    """nq needle descriptors: fresh palettes, and entries of the index with their colours moved a little"""
    import color_search_cases as CS

    rng = np.random.default_rng([seed, 37])
    nd, _ = CS.synth_descriptors(nq, seed % 100000 + 7)
    live = np.flatnonzero(m.ids != 0)
    for j in range(nq):
        if len(live) and rng.random() < 0.6:
            nd[j] = m.d[int(rng.choice(live))]
            k = int(nd[j]["numColors"])
            if k and rng.random() < 0.7:
                nd[j]["colors"][:k] = np.clip(nd[j]["colors"][:k].astype(np.int64) + rng.integers(-300, 301, (k, 4)), 0, 65535)
    return nd


def _resolve_color(world, op, m):
    import color_search_cases as CS

    name = op[0]
    if name == "add":
        return {"d": CS.synth_descriptors(op[2], op[3])[0], "ids": world.take_ids(op[2])}
    if name == "add_refused":
        n = m.count() // 2 + 4100  # past any capacity the growth rule can have left behind
        return {"d": CS.synth_descriptors(n, 4242)[0], "ids": np.arange(1, n + 1, dtype=np.uint32) + np.uint32(1 << 30)}
    if name == "remove":
        return {"ids": _remove_ids(world, m, op[2])}
    if name == "slice":
        if op[4]:
            return {"ids": _slice_ids(world, m, op)}
        rng = np.random.default_rng([op[2], 13])
        live = m.live_ids()
        return {"ids": np.concatenate([np.sort(rng.choice(live, min(op[3], len(live)), replace=False)), [world.next_id + 9]]).astype(np.uint32)}
    if name == "find":
        nd = _color_needles(m, op[2], 4)
        return {"d": nd[nd["numColors"] > 0][0] if (nd["numColors"] > 0).any() else nd[0]}
    if name == "find_by_id":
        live = m.live_ids()
        return {"id": int(np.random.default_rng([op[2], 23]).choice(live)) if len(live) else world.next_id + 3}
    if name in ("find_batch", "distances"):
        return {"d": _color_needles(m, op[2], op[3])}
    if name == "sort_similar":  # a selection: ids of the index in a drawn order, and two it does not hold
        rng = np.random.default_rng([op[2], 41])
        live = m.live_ids()
        sel = rng.choice(live, min(op[3], len(live)), replace=False) if len(live) else live
        return {"ids": np.concatenate([sel, [world.next_id + 1, world.next_id + 2]]).astype(np.uint32)}
    return {}


def _expect_color(op, a, m):
    import color_search_cases as CS
    from sort_similar_table_rules import color_table, table_model

    from oracle import ColorOracle

    name = op[0]
    if name in ("find", "find_by_id"):
        if name == "find_by_id":  # findIndexData: the first entry with that id; no entry, or one without colours: nothing
            pos = np.flatnonzero(m.ids == a["id"])
            if not len(pos) or a["id"] == 0 or m.d[pos[0]]["numColors"] == 0:
                return []
            target = m.d[pos[0]]
        else:
            target = a["d"]
        if m.count() == 0 or target["numColors"] == 0:
            return []
        return _pairs(*ColorOracle().find(m.d, m.ids, target))
    if name == "find_batch":
        if m.count() == 0:
            return reference_empty(len(a["d"]), op[4])
        return CS.reference_cut(CS.np_scores(a["d"], m.d), m.ids, op[4])
    if name == "distances":
        return CS.np_scores(a["d"], m.d).view(np.uint32) if m.count() else np.zeros((len(a["d"]), 0), np.uint32)
    if name == "sort_similar":
        ids = a["ids"]
        where = {int(i): k for k, i in enumerate(m.ids.tolist()) if i}
        in_index = np.array([int(i) in where for i in ids], np.uint8)
        entry = np.zeros(len(ids), CS.COLOR_DTYPE)
        for k, i in enumerate(ids.tolist()):
            if in_index[k]:
                entry[k] = m.d[where[i]]
        return [list(table_model(color_table(entry, entry, CS.np_scores, CS.int_scores), ids, 1, 5, in_index))]
    if name == "download":
        return m.ids, m.d.tobytes()
    raise ValueError(op)


def reference_empty(nq, k):
    return np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.int32), np.zeros(nq, np.uint32)


def canon(x):
    """arrays, tuples and lists of them as plain nested lists, for == and for printing"""
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, (tuple, list)):
        return [canon(y) for y in x]
    if isinstance(x, np.generic):
        return x.item()
    return x


def apply_mutation(world, op, a):
    """the mirror's side of a mutation; -> True when the handle's contents changed (what cbh_idx64::contents_changed sees)"""
    name, m = op[0], world.handles[op[1]]
    if name == "load":
        m.load(a["h"], a["ids"])
        return True
    if name == "add" and world.kind == "color":
        m.add(a["d"], a["ids"])
        return True
    if name == "add":
        m.add(a["h"], a["ids"])
        return len(a["h"]) > 0
    if name == "remove":
        changed = len(a["ids"]) > 0 and m.count() > 0  # (idx_remove returns early otherwise)
        m.remove(a["ids"])
        return changed
    if name == "slice":
        world.handles.append(m.slice(a["ids"]))
    elif name == "set_record_capacity":
        m.rec_cap = op[2]
    elif name == "join_prepare":
        m.opted = True
    elif name == "join_release":
        m.opted = False
    return False  # (add_refused: nothing at all)


# ---- hand-written sequences: every boundary once, in a fixed order ----------------------------------------------------
HAND = {
    "dcthash": [
        ("load", 0, 1000, 1, None),             # 1000 slots: capacity 1024
        ("find_batch", 0, 2, 64, 5, 10),        # the counting select; the workspace's first record block (2^24)
        ("find_batch", 0, 2, 64, 5, 10),        # the same again: tables and workspace reused
        ("add", 0, 1, 3),                       # 1001: inside the capacity
        ("find", 0, 4, 5),                      # the lone-needle block
        ("add", 0, 30, 5),                      # 1031: across 1024 -> 2048, device-to-device copy of 1001 rows
        ("download", 0),                        # every row survived the copy, the last one included
        ("find_batch", 0, 6, 64, 8, 65),        # the sort path (k > 64)
        ("slice", 0, 7, 1, 2),                  # handle 1: half of the ids, taken BEFORE the parent grows
        ("find_batch", 0, 6, 64, 8, 10),        # the parent right after the slice
        ("set_record_capacity", 1, 1024),       # the slice's first record block will hold 1024 records
        ("add", 0, 1023, 8),                    # 2054: across 2048 -> 3072
        ("find_batch", 0, 9, 64, 4, 10),        # the parent after the growth
        ("add", 1, 6000, 26),                   # the slice, loaded to fit (515 of capacity 1024), grows to 6515
        ("find_batch", 1, 9, 64, 8, 10),        # the slice: more than 1024 records, scan_all grows and scans again
        ("find_batch", 1, 9, 64, 8, 65),        # and its sort buffers are sized after the grown block
        ("set_record_capacity", 1, REC_CAP_DEFAULT),
        ("find_batch", 1, 9, 64, 5, 10),
        ("add", 1, 200, 10),                    # the slice grows on its own
        ("find_masked", 1, 11, 48, 6, 10),
        ("remove", 0, ("draw", 12, 150)),       # live, removed, absent and repeated ids
        ("cluster_labels", 0, 3),
        ("cluster_labels", 0, 3),
        ("find_batch", 0, 9, 64, 4, 10),        # the needles of the search before the remove: removed entries are gone
        ("find_masked", 0, 13, 64, 5, 10),      # a remove between a plain and a masked search
        ("set_record_capacity", 0, 1024),       # the parent's block is 2^24 records and stays ...
        ("cluster_labels", 0, 3),               # ... until cluster_labels gives back what is above max(1024, 2^22)
        ("find_batch", 0, 9, 64, 8, 10),        # a block of 1024, more than 1024 records: grown and scanned again
        ("find_batch", 0, 9, 64, 8, 65),
        ("set_record_capacity", 0, REC_CAP_DEFAULT),
        ("join_prepare", 0, 5),
        ("find_batch", 0, 14, 64, 5, 10),
        ("remove", 0, ("draw", 12, 150)),       # the same ids again: all of them removed already
        ("search_index_batch", 0, 15, 48, 2, 6, 1, 5),  # escalation from threshold 2 to 6
        ("search_index_batch", 0, 15, 48, 2, 6, 1, 5),
        ("find_batch", 0, 14, 64, 5, 10),
        ("find_coalesced", 0, 16, 24, 5),       # combined scans, later the self-join snapshot of this generation
        ("find_coalesced", 0, 16, 24, 5),
        ("add", 0, 1500, 17),                   # 3554: across 3072 -> 4608; the snapshot is one generation old
        ("find_coalesced", 0, 16, 24, 5),
        ("find", 0, 18, 30),                    # more than 512 matches: past the lone-needle block, scan_all, host sort
        ("find", 0, 18, 30),
        ("join_release", 0),
        ("find_batch", 0, 19, 64, 8, 10),
        ("add_refused", 0),                     # CBH_E_NOMEM: reserve() keeps the old arrays
        ("download", 0),
        ("find_batch", 0, 19, 64, 8, 10),
        ("remove", 0, ("all",)),                # everything at once ...
        ("find_batch", 0, 19, 64, 8, 10),       # ... nothing is found ...
        ("add", 0, 30, 20),                     # ... then an add behind 3554 dead slots
        ("find_batch", 0, 21, 32, 8, 10),
        ("download", 0),
        ("load", 0, 1200, 22, None),            # load on a loaded handle: a reload into the capacity that is there
        ("find_batch", 0, 23, 64, 5, 65),
        ("download", 0),
        ("remove", 1, ("draw", 24, 40)),        # the slice is still alive and its own
        ("find_batch", 1, 25, 64, 5, 10),
        ("download", 1),
    ],
    # the HammingTree's shape of a DctHashIndex: remove() zeroes hashes, which moves values to prefix 0
    "dcthash_tree": [
        ("load", 0, 16000, 30, 7900),           # 7900 hashes with bit 0 set, 8100 without: root internal, two leaves
        ("tree_masks", 0, 31, 64),              # every needle: mask 1
        ("find_masked", 0, 31, 64, 6, 10),
        ("remove", 0, ("range", 1, 201)),       # 200 of the bit-0 hashes become 0: 8300 values under prefix 0
        ("tree_masks", 0, 31, 64),              # needles with bit 0 clear: mask 3
        ("find_masked", 0, 31, 64, 6, 10),
        ("find_masked", 0, 31, 64, 6, 10),
    ],
    "fdct": [
        ("load", 0, 100, 10, 1),                # 1000 values: capacity 1024
        ("find_batch", 0, 2, 8, 5),
        ("find_batch", 0, 2, 8, 5),
        ("add", 0, 1, 1, 3),                    # 1001
        ("find", 0, 4, 6),
        ("add", 0, 3, 10, 5),                   # 1031: across 1024
        ("download", 0),
        ("find_by_id", 0, 6, 6),                # the needle's hashes come from the index (hashesForId)
        ("slice", 0, 7, 1, 2),                  # handle 1
        ("find_batch", 0, 2, 8, 5),             # the parent right after the slice
        ("set_record_capacity", 1, 1024),
        ("add", 0, 93, 11, 8),                  # 2054: across 2048
        ("find_batch", 0, 9, 8, 8),
        ("add", 1, 600, 10, 29),                # the slice grows before its first search
        ("find_batch", 1, 9, 8, 9),             # the slice: more than 1024 records into a block of 1024
        ("set_record_capacity", 1, REC_CAP_DEFAULT),
        ("find", 1, 11, 6),
        ("add", 1, 20, 10, 10),
        ("find", 1, 11, 6),
        ("remove", 0, ("draw", 12, 20)),        # ids zeroed, hashes kept: the tables go, the tree stays
        ("hashes_for_id", 0, 14),
        ("hashes_for_id", 0, 14),
        ("find_batch", 0, 9, 8, 8),
        ("tree_masks", 0, 13, 32),
        ("join_prepare", 0, 8),
        ("find_batch", 0, 15, 8, 8),
        ("remove", 0, ("draw", 16, 20)),
        ("find_batch", 0, 15, 8, 8),
        ("find_batch", 0, 15, 8, 8),
        ("join_release", 0),
        ("find_batch", 0, 15, 8, 8),
        ("add", 0, 150, 10, 17),                # 3554: across 3072
        ("find_by_id", 0, 18, 6),
        ("find_by_id", 0, 18, 6),
        ("add_refused", 0),
        ("download", 0),
        ("find", 0, 19, 6),
        ("find", 0, 19, 6),
        ("remove", 0, ("all",)),
        ("find_batch", 0, 15, 8, 8),            # every id is 0: votes for nobody
        ("add", 0, 3, 10, 20),
        ("find_batch", 0, 21, 6, 8),
        ("load", 0, 80, 100, 22),               # 8000 values: the tree is one leaf
        ("tree_masks", 0, 23, 32),
        ("find_batch", 0, 24, 8, 4),
        ("add", 0, 3, 100, 25),                 # 8300 values: the root is internal, every needle sees one half
        ("tree_masks", 0, 23, 32),
        ("find_batch", 0, 24, 8, 4),
        ("tree_masks", 0, 23, 32),
        ("load", 0, 80, 100, 26),               # back to 8000: one leaf again
        ("tree_masks", 0, 23, 32),
        ("find_batch", 0, 24, 8, 4),
        ("remove", 1, ("draw", 27, 5)),
        ("find_batch", 1, 28, 8, 6),
        ("download", 1),
    ],
}
HAND["fdct_tree"] = HAND["fdct"]
HAND["color"] = [
    ("add", 0, 4000, 1),                    # 4000 entries: planes of 4096
    ("find_batch", 0, 2, 8, 5),
    ("find_batch", 0, 2, 8, 5),
    ("add", 0, 30, 3),                      # 4030: inside the planes
    ("find", 0, 4),
    ("slice", 0, 5, 255, 0),                # handle 1: 255 entries, planes of 256, taken before the parent grows
    ("find_batch", 0, 6, 8, 10),            # the parent right after the slice
    ("add", 0, 200, 7),                     # 4230: across 4096 -> 10240, hipMemcpy2D by the old pitch
    ("download", 0),
    ("distances", 0, 8, 6),                 # every plane survived the copy: floats, bit for bit
    ("distances", 0, 8, 6),
    ("slice", 1, 9, 128, 0),                # handle 2: 128 of 255 kept, no slack at all
    ("add", 2, 1, 10),                      # ... so this add grows the planes
    ("find_batch", 2, 11, 8, 5),
    ("add", 2, 8, 12),
    ("distances", 2, 13, 6),
    ("slice", 1, 14, 7, 0),                 # handle 3: 7 entries
    ("slice", 3, 15, 3, 0),                 # handle 4: 3 of 7 kept, planes of 4
    ("add", 4, 1, 16),                      # lands on the padding entry
    ("find", 4, 17),
    ("add", 4, 8, 18),                      # and now grows
    ("find_batch", 4, 19, 4, 5),
    ("download", 4),
    ("remove", 0, ("draw", 20, 150)),       # live, removed, absent and repeated ids
    ("find_by_id", 0, 21),
    ("find_by_id", 0, 21),
    ("sort_similar", 0, 22, 40),
    ("sort_similar", 0, 22, 40),
    ("remove", 1, ("draw", 23, 20)),        # the first slice is still its own
    ("sort_similar", 1, 24, 24),
    ("add_refused", 0),                     # CBH_E_NOMEM: nothing of the refused entries may stay behind ...
    ("find_batch", 0, 25, 8, 5),
    ("add", 0, 30, 26),                     # ... or this add would upload THEM instead of its own
    ("find_batch", 0, 27, 8, 5),
    ("download", 0),
    ("add", 0, 6100, 28),                   # 10360: across 10240 -> 19456
    ("find", 0, 29),
    ("find", 0, 29),
    ("distances", 0, 30, 4),
    ("remove", 0, ("all",)),
    ("find_batch", 0, 27, 8, 5),            # nothing is found
    ("add", 0, 30, 31),
    ("find_batch", 0, 32, 8, 5),
    ("download", 0),
    ("download", 0),
]


# the regression of cbh_color_add (NOTES.md section 32): the refused entries stayed in the host copies, and the next add
# uploaded them in place of its own
HAND["color_refused_add_leaves_nothing_behind"] = [
    ("add", 0, 100, 1),
    ("find_batch", 0, 2, 8, 5),
    ("add_refused", 0),
    ("find_batch", 0, 2, 8, 5),             # as before the call
    ("add", 0, 30, 3),
    ("find_batch", 0, 4, 8, 5),             # the 30 new entries answer, not the refused ones
    ("distances", 0, 5, 6),
    ("download", 0),
]


# ---- the generator ----------------------------------------------------------------------------------------------------
def _search(kind, rng, t, route=None, joined=False):
    routes = ROUTES[kind]
    route = route or routes[int(rng.integers(0, len(routes)))]
    s = int(rng.integers(1, 1 << 20))
    th = int(rng.choice(JOIN_THRESHOLDS)) if joined or rng.random() < 0.5 else int(rng.integers(2, 10))
    nq = int(rng.choice([1, 7, 33, 64]))
    if kind == "dcthash":
        return {"find": ("find", t, s, int(rng.choice([th, 30]))),
                "find_batch": ("find_batch", t, s, 64, th, 10),
                "find_batch65": ("find_batch", t, s, 64, th, 65),
                "find_masked": ("find_masked", t, s, nq, th, 10),
                "search_index_batch": ("search_index_batch", t, s, nq, 2, int(rng.choice([0, 6])), 1, 5),
                "find_coalesced": ("find_coalesced", t, s, 16, th),
                "cluster_labels": ("cluster_labels", t, int(rng.choice([1, 3]))),
                "download": ("download", t)}[route]
    return {"find": ("find", t, s, th), "find_by_id": ("find_by_id", t, s, th),
            "find_batch": ("find_batch", t, s, int(rng.choice([1, 5, 8])), th),
            "hashes_for_id": ("hashes_for_id", t, s), "tree_masks": ("tree_masks", t, s, nq),
            "download": ("download", t)}[route]


def _add(kind, rng, t, n):
    s = int(rng.integers(1, 1 << 20))
    if kind == "dcthash":
        return ("add", t, n, s)
    k = 11 if n % 11 == 0 and n > 30 else 10 if n % 10 == 0 else 1
    return ("add", t, n // k, k, s)


def _mutation(kind, rng, t, name):
    s = int(rng.integers(1, 1 << 20))
    if name == "load":
        return ("load", t, 700, s, None) if kind == "dcthash" else ("load", t, 70, 10, s)
    if name == "add":
        return _add(kind, rng, t, int(rng.choice([1, 30, 200])))
    if name == "remove":
        return ("remove", t, ("draw", s, int(rng.integers(1, 120))))
    if name == "set_record_capacity":
        return ("set_record_capacity", t, int(rng.choice([4096, REC_CAP_DEFAULT])))
    if name == "join_prepare":
        return ("join_prepare", t, int(rng.choice(JOIN_THRESHOLDS)))
    if name == "join_release":
        return ("join_release", t)
    if name == "add_refused":
        return ("add_refused", t)
    raise ValueError(name)


def _search_color(rng, t, route=None):
    routes = ROUTES["color"]
    route = route or routes[int(rng.integers(0, len(routes)))]
    s = int(rng.integers(1, 1 << 20))
    return {"find": ("find", t, s), "find_by_id": ("find_by_id", t, s),
            "find_batch": ("find_batch", t, s, int(rng.choice([1, 5, 8])), int(rng.choice([1, 5, 10]))),
            "distances": ("distances", t, s, int(rng.choice([1, 6]))),
            "sort_similar": ("sort_similar", t, s, int(rng.choice([2, 24, 40]))), "download": ("download", t)}[route]


def _sequence_color(seed, steps):
    rng = np.random.default_rng(seed)
    sd = lambda: int(rng.integers(1, 1 << 20))  # noqa: E731
    srch = lambda t, r=None: _search_color(rng, t, r)  # noqa: E731

    def mut(t, name):
        return {"add": ("add", t, int(rng.choice([1, 30])), sd()), "remove": ("remove", t, ("draw", sd(), int(rng.integers(1, 120)))),
                "add_refused": ("add_refused", t)}[name]

    plain = ("add", "remove", "add_refused")
    segs = []
    for route in ROUTES["color"]:
        segs.append(lambda t, new, r=route: [mut(t, plain[int(rng.integers(0, 3))]), srch(t, r), srch(t, r)])
    for name in plain:
        segs.append(lambda t, new, n=name: [mut(t, n), srch(t)])
    for n in (200, 6200):  # across 4096, and across the next growth
        segs.append(lambda t, new, n=n: [("add", 0, n, sd()), srch(0), srch(0, "distances"), srch(0, "download")])
    segs.append(lambda t, new: [("remove", t, ("all",)), srch(t), ("add", t, 30, sd()), srch(t)])
    segs.append(lambda t, new: [("add_refused", t), ("add", t, 30, sd()), srch(t, "find_batch"), srch(t, "download")])
    segs.append(lambda t, new: [("slice", t, sd(), 1, 2), srch(t), ("add", t, 30, sd()), srch(t), ("add", new, 30, sd()), srch(new)])
    for total, kept in ((7, 3), (255, 128)):  # the two slices tests/test_slice_device.py names, each added to afterwards
        segs.append(lambda t, new, a=total, b=kept: [("slice", 0, sd(), a, 0), srch(0), ("slice", new, sd(), b, 0),
                                                     ("add", new + 1, 1, sd()), srch(new + 1, "find_batch"),
                                                     ("add", new + 1, 8, sd()), srch(new + 1, "distances"), srch(new + 1, "download")])
    ops, handles = [("add", 0, 4000, sd())], 1
    order = [int(i) for i in rng.permutation(len(segs))]
    order.sort(key=lambda i: 9 <= i <= 10)  # (stable: the two large adds last -- the oracle's work grows with the index)
    for i in order:
        t = 0 if rng.random() < 0.7 else int(rng.integers(0, handles))
        for op in segs[i](t, handles):
            handles += op[0] == "slice"
            ops.append(op)
    while len(ops) < steps:
        ops.append(srch(0))
    return ops


def sequence(kind, seed, steps=40):
    """A list of at least `steps` ops for `kind` from np.random.default_rng(seed).  Made of short segments in a drawn
    order -- a mutation and a search, a mutation and the same search twice, the four capacity adds, a slice whose two
    sides are then used, remove-all-then-add, a small record block and a large result -- so that the conditions of
    tests/test_index_sequences_model.py hold for most seeds; the seeds in use are the ones for which they all do."""
    if kind == "color":
        return _sequence_color(seed, steps)
    if kind in ("cv", "cv_sharded"):  # (the other two handle classes have modules of their own)
        import index_sequences_cv

        return index_sequences_cv.sequence(kind, seed, steps)
    if kind == "video":
        import index_sequences_video

        return index_sequences_video.sequence(seed, steps)
    rng = np.random.default_rng(seed)
    first = ("load", 0, 1000, int(rng.integers(1, 1 << 20)), None) if kind == "dcthash" else \
        ("load", 0, 100, 10, int(rng.integers(1, 1 << 20)))
    plain = [m for m in MUTATIONS if m != "slice"]
    segs = []
    for route in ROUTES[kind]:  # every route right after a mutation, then again
        name = plain[int(rng.integers(0, len(plain)))]
        segs.append(lambda t, n=name, r=route: [_mutation(kind, rng, t, n), _search(kind, rng, t, r), _search(kind, rng, t, r)])
    for name in plain:  # every mutation followed by a search
        segs.append(lambda t, n=name: [_mutation(kind, rng, t, n), _search(kind, rng, t)])
    for n in (1, 30, 1023, 1500, 1500):  # the capacity adds (on handle 0 whatever t is)
        segs.append(lambda t, n=n: [_add(kind, rng, 0, n), _search(kind, rng, 0), _search(kind, rng, 0, "download")])
    segs.append(lambda t: [("remove", t, ("all",)), _search(kind, rng, t), _add(kind, rng, t, 30), _search(kind, rng, t)])
    def big(t):  # a find_batch with more records than a block of 1024 holds
        s = int(rng.integers(1, 1 << 20))
        return ("find_batch", t, s, 64, 8, 10) if kind == "dcthash" else ("find_batch", t, s, 8, 9)

    segs.append(lambda t: ["SLICE", _search(kind, rng, t), ("set_record_capacity", "NEW", SMALL_REC_CAP),
                           _add(kind, rng, "NEW", 6000), big("NEW"), big("NEW"),
                           ("set_record_capacity", "NEW", REC_CAP_DEFAULT),
                           _add(kind, rng, t, 200), _search(kind, rng, t), _add(kind, rng, "NEW", 30), _search(kind, rng, "NEW")])
    if kind == "dcthash":  # a block dropped under a small capacity on the handle of the start, grown again by the next result
        segs.append(lambda t: [("set_record_capacity", 0, SMALL_REC_CAP), ("cluster_labels", 0, 3), big(0),
                               ("find_batch", 0, int(rng.integers(1, 1 << 20)), 64, 8, 65), ("set_record_capacity", 0, REC_CAP_DEFAULT),
                               _search(kind, rng, 0)])
    for th in JOIN_THRESHOLDS:  # the three join kernels: a search, a remove that keeps the size, the search again
        segs.append(lambda t, th=th: [_retarget(_search(kind, rng, t, "find_batch", joined=True), th),
                                      ("remove", t, ("draw", int(rng.integers(1, 1 << 20)), 60)),
                                      _retarget(_search(kind, rng, t, "find_batch", joined=True), th)])
    ops, handles = [first], 1
    for i in rng.permutation(len(segs)):
        t = 0 if rng.random() < 0.7 else int(rng.integers(0, handles))
        new = handles
        for op in segs[int(i)](t):
            if op == "SLICE":
                op = ("slice", t, int(rng.integers(1, 1 << 20)), 1, 2)
                handles += 1
            ops.append(tuple(new if x == "NEW" else x for x in op))
    while len(ops) < steps:
        ops.append(_search(kind, rng, 0))
    return ops


def _retarget(op, thresh):
    """a find_batch op at another threshold (position 4 for both kinds)"""
    return op[:4] + (thresh,) + op[5:]


class RescanRule:
    """Where scan_all MUST find its record block too small, grow it and scan again -- told from the ops alone, so that the
    device tests can ask the handle's counters whether it did (cbh_idx64_get_stats: one scan launch per attempt;
    cbh_idx64_shard_stats: rescans).  A workspace keeps the largest block it ever had, so "rec_cap_default is 1024" is not
    enough; the block is known to be 1024 records
      plain handle    when the find_batch is the handle's first search, or follows a cluster_labels that ran under the small
                      capacity (clusters.hip settle() gives a block above max(rec_cap_default, 2^22) back);
      sharded handle  when it is the first search since set_record_capacity(1024): a shard's default block (2^24) is above
                      what ~ShardLeases lets it keep (2^22) and is dropped after every search, and some shard has more
                      than 1024 of the records when there are more than 1024 per shard on average."""

    def __init__(self):
        self.last_search, self.since_small = {}, {}

    def mutation(self, op):
        if op[0] == "set_record_capacity":
            self.since_small[op[1]] = 0

    def must(self, op, m, records, shards=1):
        t = op[1]
        if op[0] != "find_batch" or m.rec_cap != SMALL_REC_CAP:
            return False
        if shards > 1:
            return records > SMALL_REC_CAP * shards and self.since_small.get(t) == 0
        return records > SMALL_REC_CAP and self.last_search.get(t, ("cluster_labels", SMALL_REC_CAP)) == ("cluster_labels", SMALL_REC_CAP)

    def search(self, op, m):
        self.last_search[op[1]] = (op[0], m.rec_cap)
        self.since_small[op[1]] = self.since_small.get(op[1], 0) + 1


# ---- coverage: conditions on a sequence, from the mirror alone --------------------------------------------------------
def coverage(kind, ops):
    """walk `ops` on the mirror (no oracle, no device) and say what the sequence exercises: a dict of facts that
    tests/test_index_sequences_model.py turns into assertions"""
    world = World(kind)
    facts = {"ops": len(ops), "crossings0": None, "mutation_then_search": set(), "route_after_mutation": set(),
             "route_second_in_row": set(), "slice_parent_used": False, "slice_itself_used": False,
             "remove_all_then_add": False, "rescans": 0, "rescans_shards5": 0, "rescans_parent": 0, "join_thresholds": set(), "max_needles": 0, "max_slots": 0,
             "tree_kinds": set(), "stale_join_chances": 0, "slices_added_to": set(), "refused_then_add": False}
    kept_of, refused, added_after_refusal = {}, set(), set()
    parents, mutated_after_slice = {}, {}
    rule = RescanRule()
    prev = None
    removed_all = set()
    joined_since = {}  # handle -> thresholds of find_batch since its last content mutation
    for op in ops:
        t = op[1]
        m = world.handles[t]
        a = resolve(world, op)
        if is_search(op):
            r = route_of(op)
            if prev is not None and prev[1] == t:
                if is_search(prev):
                    facts["route_second_in_row"].add(r)
                else:
                    facts["mutation_then_search"].add(prev[0])
                    facts["route_after_mutation"].add(r)
            for key in ("q", "needles", "d"):
                if key in a and (isinstance(a[key], list) or getattr(a[key], "ndim", 0)):
                    facts["max_needles"] = max(facts["max_needles"], len(a[key]))
            if t in mutated_after_slice and mutated_after_slice[t]:
                facts["slice_itself_used" if t in parents else "slice_parent_used"] = True
            if t in added_after_refusal:
                facts["refused_then_add"] = True
            if kind != "color" and op[0] == "find_batch":
                th = op[4]
                if th in JOIN_THRESHOLDS:
                    facts["join_thresholds"].add(th)
                    if th in joined_since.get(t, {}).get("after_remove", ()):
                        facts["stale_join_chances"] += 1
                    joined_since.setdefault(t, {"seen": set(), "after_remove": set()})["seen"].add(th)
                if m.rec_cap == SMALL_REC_CAP:
                    n_rec = _records(world.kind, m, a, th)
                    facts["rescans"] += rule.must(op, m, n_rec)
                    facts["rescans_parent"] += rule.must(op, m, n_rec) and t not in parents
                    facts["rescans_shards5"] += rule.must(op, m, n_rec, 5)
            if kind != "color":
                rule.search(op, m)
            if kind != "color" and (op[0] in ("tree_masks", "find_masked") or kind == "fdct_tree"):
                facts["tree_kinds"].add("internal" if m.count() > TREE_LEAF else "leaf")
        else:
            rule.mutation(op)
            if op[0] == "add_refused":
                refused.add(t)
            if op[0] == "add" and t in refused:
                added_after_refusal.add(t)
            if op[0] == "add" and t in kept_of:
                facts["slices_added_to"].add(kept_of[t])
            if op[0] == "slice":
                kept_of[len(world.handles)] = (m.count(), int(np.isin(m.ids, a["ids"]).sum()))
                mutated_after_slice[t] = False
                mutated_after_slice[len(world.handles)] = False
                parents[len(world.handles)] = t
            if op[0] in CONTENT_MUTATIONS:
                if t in mutated_after_slice:
                    mutated_after_slice[t] = True
                if op[0] == "add" and t in removed_all:
                    facts["remove_all_then_add"] = True
                removed_all.discard(t)
                if op[0] == "remove" and op[2] == ("all",) and m.count():
                    removed_all.add(t)
                js = joined_since.setdefault(t, {"seen": set(), "after_remove": set()})
                # a remove keeps the slot count: the one mutation after which a table that was not dropped still fits
                js["after_remove"] = set(js["seen"]) if op[0] == "remove" else set()
                js["seen"] = set()
            apply_mutation(world, op, a)
            facts["max_slots"] = max(facts["max_slots"], max(h.count() for h in world.handles))
        prev = op
    facts["crossings0"] = list(world.handles[0].crossings)
    return facts


def _records(kind, m, a, thresh):
    """records a find_batch leaves in the workspace: pairs under the threshold (numpy, not the oracle)"""
    if kind == "dcthash":
        q = a["q"][a["q"] != 0]
        live = (m.ids != 0) & (m.h != 0)
        return int((np.bitwise_count(q[:, None] ^ m.h[live][None, :]) < thresh).sum())
    q = np.concatenate([kp for _, kp in a["needles"]])
    return int((np.bitwise_count(q[:, None] ^ m.h[None, :]) < thresh).sum())  # (keep_id0: removed entries count)


def paste(kind, seed, ops):
    """a failing prefix in the form of a hand-written sequence"""
    lines = "\n".join(f"    {op!r}," for op in ops)
    return f"# kind {kind!r}, seed {seed!r}, failed at step {len(ops) - 1}\n[\n{lines}\n]"
