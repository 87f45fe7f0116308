"""Long-lived index handles on sequences of mutations and searches (tests/index_sequences.py: DctHashIndex,
DctFeaturesIndex, ColorDescIndex; tests/index_sequences_cv.py: CvFeaturesIndex; tests/index_sequences_video.py:
DctVideoIndex): every sequence runs against the real handle and the host mirror in lockstep, and after every search the
handle's answer equals the mirror's record for record -- ids, scores or distances, counts, order.  Everything is integer
(the colour distances are compared as bit patterns): there is no tolerance.

What the sequences go after is the state a handle derives from its contents and keeps between calls (NOTES.md section 32,
"State a handle keeps between calls"): capacity growth with its device-to-device copy, the join's resident slot tables,
the HammingTree shape, the coalescer's self-join snapshot, the workspace's record and sort blocks, the lone-needle block,
the video index's built structure and its skipFrames, the 256-bit shards' segment tables, the colour planes.

The seeds are the ones tests/test_index_sequences_model.py asserts the coverage conditions for.

A failure prints the kind, the seed, the step and the ops up to and including the failing one as a list that can be
pasted back as a hand-written sequence.  After every sequence the handles are destroyed and "arena_live_bytes" -- the
key tests/test_error_paths.py uses for leaks; there is no "live_bytes" key -- is what it was before.
"""
import ctypes as C
import gc
import warnings

import numpy as np
import pytest

import index_sequences as S
import index_sequences_cv as V
import index_sequences_video as W

# chosen on the CPU by tests/test_index_sequences_model.py::test_the_seeds_in_use_meet_every_condition
SEEDS = {"dcthash": (1, 7, 8), "fdct": (2, 4, 8), "fdct_tree": (2, 4, 8), "color": (1, 2, 3), "cv": (1, 2, 3),
         "cv_sharded": (1, 2, 3), "video": (1, 2, 3)}
HAND = {"dcthash": ("dcthash", "dcthash_tree"), "fdct": ("fdct",), "fdct_tree": ("fdct_tree",), "color": ("color", "color_refused_add_leaves_nothing_behind"),
        "cv": ("cv",), "cv_sharded": ("cv_sharded",)}


def cases(kind):
    """(name of the sequence, its ops) for every sequence of `kind` the device tests run"""
    if kind == "video":
        return [(f"seed{s}", W.sequence(s)) for s in SEEDS[kind]] + [("hand_video", W.HAND)]
    mod = V if kind in V.KINDS else S
    return [(f"seed{s}", mod.sequence(kind, s)) for s in SEEDS[kind]] + [(f"hand_{h}", mod.HAND[h]) for h in HAND[kind]]


def _names(kind):
    return [n for n, _ in cases(kind)]


def _tuning(L, key):
    v = C.c_longlong(-2)
    assert L.cbh_get_tuning(key, C.byref(v)) == 0, key
    return int(v.value)


def _p(a):
    return a.ctypes.data if len(a) else None


def _u64(a):
    return np.ascontiguousarray(a, np.uint64)


def _u32(a):
    return np.ascontiguousarray(a, np.uint32)


class Real:
    """the device side of a sequence: one DctHashIndex / DctFeaturesIndex per handle number"""

    def __init__(self, gpu, kind):
        from cbird_amd import _lib

        self.gpu, self.kind, self._lib, self.L = gpu, kind, _lib, _lib.lib()
        if kind == "dcthash":
            first = gpu.DctHashIndex()
        else:
            first = gpu.DctFeaturesIndex(tree_compat=kind == "fdct_tree")
        self.idx = [first]
        self.shards = int(self.L.cbh_idx64_shard_count(first.handle))
        self.sharded = self.shards > 1
        self.self_join_on = set()

    def close(self):
        self.idx.clear()
        gc.collect()

    # -- mutations ------------------------------------------------------------------------------------------------------
    def mutate(self, op, a):
        L, check = self.L, self._lib.check
        name, ix = op[0], self.idx[op[1]]
        if name == "load":  # (the C call: on a loaded handle it reloads; the Python wrapper keeps `if (!isLoaded())`)
            h, ids = _u64(a["h"]), _u32(a["ids"])
            check(L.cbh_idx64_load(ix.handle, _p(h), _p(ids), len(h)), "load")
        elif name == "add":
            h, ids = _u64(a["h"]), _u32(a["ids"])
            check(L.cbh_idx64_add(ix.handle, _p(h), _p(ids), len(h)), "add")
        elif name == "add_refused":
            if self.sharded:
                return  # (what a partial failure leaves behind on a sharded handle is not a rule: the op is left out)
            h, ids = _u64(a["h"]), _u32(a["ids"])
            fired0 = _tuning(L, b"fault_fired")
            L.cbh_set_tuning(b"fault_alloc_after", 0)
            try:
                rc = L.cbh_idx64_add(ix.handle, _p(h), _p(ids), len(h))
            finally:
                L.cbh_set_tuning(b"fault_alloc_after", -1)
            assert rc == self._lib.CBH_E_NOMEM and _tuning(L, b"fault_fired") == fired0 + 1, rc
            self._lib.lib().cbh_clear_error()
        elif name == "remove":
            ids = _u32(a["ids"])
            f = L.cbh_idx64_remove if self.kind == "dcthash" else L.cbh_idx64_remove_ids_only
            check(f(ix.handle, _p(ids), len(ids)), "remove")
        elif name == "slice":
            self.idx.append(ix.slice(a["ids"].tolist()))
        elif name == "set_record_capacity":
            check(L.cbh_idx64_set_record_capacity(ix.handle, op[2]), "set_record_capacity")
        elif name == "join_prepare":
            ix.join_prepare(op[2])
        elif name == "join_release":
            ix.join_release()
        else:
            raise ValueError(op)

    def scan_attempts(self, ix):
        """what grows with every attempt of scan_all: a plain handle counts its scan launches, a sharded one its rescans"""
        if self.sharded:
            sh = self._lib.cbh_shard_stats()
            self._lib.check(self.L.cbh_idx64_shard_stats(ix.handle, C.byref(sh)), "shard_stats")
            return int(sh.rescans)
        st = self._lib.cbh_stats()
        self._lib.check(self.L.cbh_idx64_get_stats(ix.handle, C.byref(st)), "get_stats")
        return int(st.scan_launches)

    # -- searches -------------------------------------------------------------------------------------------------------
    def _download(self, ix):
        n = ix.count()
        h, ids = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        self._lib.check(self.L.cbh_idx64_download(ix.handle, _p(h), _p(ids), n), "download")
        return h, ids

    def _tree_masks(self, ix, q):
        q = _u64(q)
        out = np.zeros(len(q), np.uint64)
        self._lib.check(self.L.cbh_idx64_tree_masks(ix.handle, _p(q), len(q), _p(out)), "tree_masks")
        return out

    def search(self, op, a):
        gpu, L = self.gpu, self.L
        name, ix = op[0], self.idx[op[1]]
        if name == "download":
            return self._download(ix)
        if name == "tree_masks":
            return self._tree_masks(ix, a["q"])
        if self.kind == "dcthash":
            if name == "find":
                return [(x.mediaId, x.score) for x in ix.find(gpu.Media(dctHash=a["q"]), gpu.SearchParams(dctThresh=op[3]))]
            if name == "find_batch":
                return ix.find_batch(a["q"], op[4], op[5])
            if name == "find_masked":
                return ix.find_batch(a["q"], op[4], op[5], masks=ix.tree_masks(a["q"]))
            if name == "search_index_batch":
                p = gpu.SearchParams(dctThresh=op[4], maxThresh=op[5], minMatches=op[6], maxMatches=op[7], filterSelf=True)
                mi, ms, mc = ix.search_index_batch(a["q"], a["nid"], p)
                return [[(int(mi[j, t]), int(ms[j, t])) for t in range(int(mc[j]))] for j in range(len(a["q"]))]
            if name == "find_coalesced":
                if op[1] not in self.self_join_on:
                    self._lib.check(L.cbh_idx64_coalesce_set_self_join(ix.handle, 1), "self-join on")
                    self.self_join_on.add(op[1])
                cap = ix.count() + 1
                buf, n, out = (self._lib.cbh_match * cap)(), C.c_size_t(0), []
                for x in a["q"].tolist():
                    self._lib.check(L.cbh_idx64_find_coalesced(ix.handle, x, op[4], buf, cap, C.byref(n)), "find_coalesced")
                    out.append([(buf[i].id, buf[i].score) for i in range(n.value)])
                return out
            if name == "cluster_labels":
                return ix.cluster_labels(op[2])
            raise ValueError(op)
        if name in ("find", "find_by_id"):
            m = gpu.Media(id=a["id"], keyPointHashes=a["kp"].tolist())
            return [(x.mediaId, x.score) for x in ix.find(m, gpu.SearchParams(dctThresh=op[3]))]
        if name == "find_batch":
            ms = [gpu.Media(id=mid, keyPointHashes=kp.tolist()) for mid, kp in a["needles"]]
            return [[(x.mediaId, x.score) for x in r] for r in ix.find_batch(ms, gpu.SearchParams(dctThresh=op[4]))]
        if name == "hashes_for_id":
            return ix.hashesForId(a["id"])
        raise ValueError(op)


class RealColor:
    """the device side of a "color" sequence: one ColorDescIndex per handle number"""

    sharded = False

    def __init__(self, gpu):
        from cbird_amd import _lib
        from cbird_amd.colordesc import COLOR_DTYPE, ColorDescIndex

        self.gpu, self._lib, self.L, self.dtype = gpu, _lib, _lib.lib(), COLOR_DTYPE
        self.idx = [ColorDescIndex()]

    def close(self):
        self.idx.clear()
        gc.collect()

    def mutate(self, op, a):
        L = self.L
        name, ix = op[0], self.idx[op[1]]
        if name == "add":
            ids, d = _u32(a["ids"]), np.ascontiguousarray(a["d"], self.dtype)
            self._lib.check(L.cbh_color_add(ix.handle, _p(ids), _p(d), len(ids)), "add")
        elif name == "add_refused":
            ids, d = _u32(a["ids"]), np.ascontiguousarray(a["d"], self.dtype)
            fired0 = _tuning(L, b"fault_fired")
            L.cbh_set_tuning(b"fault_alloc_after", 0)
            try:
                rc = L.cbh_color_add(ix.handle, _p(ids), _p(d), len(ids))
            finally:
                L.cbh_set_tuning(b"fault_alloc_after", -1)
            assert rc == self._lib.CBH_E_NOMEM and _tuning(L, b"fault_fired") == fired0 + 1, rc
            L.cbh_clear_error()
        elif name == "remove":
            ix.remove(a["ids"].tolist())
        elif name == "slice":
            self.idx.append(ix.slice(a["ids"].tolist()))
        else:
            raise ValueError(op)

    def search(self, op, a):
        name, ix = op[0], self.idx[op[1]]
        if name in ("find", "find_by_id"):
            class M:
                id, path = a.get("id", 0), ""
                colorDescriptor = a.get("d")
            return [(x.mediaId, x.score) for x in ix.find(M)]
        if name == "find_batch":
            return ix.find_batch(a["d"], op[4])
        if name == "distances":
            return ix.distances(a["d"]).view(np.uint32)  # (bit for bit)
        if name == "sort_similar":
            p = self.gpu.SearchParams(algo=self.gpu.SearchParams.AlgoColor)
            return [list(r) for r in ix.sort_similar(a["ids"], None, p)]
        if name == "download":
            n = ix.count()
            ids, d = np.zeros(n, np.uint32), np.zeros(n, self.dtype)
            self._lib.check(self.L.cbh_color_download(ix.handle, _p(ids), _p(d), n), "download")
            return ids, d.tobytes()
        raise ValueError(op)


class _M:
    def __init__(self, id_, desc):
        self.id, self.keyPointDescriptors, self.path = id_, desc, ""


class RealCv:
    """the device side of a "cv" / "cv_sharded" sequence: one CvFeaturesIndex per handle number"""

    def __init__(self, gpu, kind):
        from cbird_amd import _lib
        from cbird_amd.cvfeatures import CvFeaturesIndex

        self.gpu, self._lib, self.L = gpu, _lib, _lib.lib()
        self.sharded = kind == "cv_sharded"
        self.idx = [CvFeaturesIndex(shards=(1, V.SHARDS)) if self.sharded else CvFeaturesIndex()]

    def close(self):
        self.idx.clear()
        gc.collect()

    def mutate(self, op, a):
        L = self.L
        name, ix = op[0], self.idx[op[1]]
        if name == "add":
            for mid, rows in zip(a["ids"].tolist(), a["rows"]):
                rows = np.ascontiguousarray(rows)
                self._lib.check(L.cbh_idx256_add(ix.handle, mid, rows.ctypes.data, len(rows)), "add")
        elif name == "add_refused":
            assert not self.sharded  # (the sharded sequences leave the op out)
            fired0 = _tuning(L, b"fault_fired")
            L.cbh_set_tuning(b"fault_alloc_after", 0)
            try:
                rc = L.cbh_idx256_add(ix.handle, a["id"], a["rows"].ctypes.data, len(a["rows"]))
            finally:
                L.cbh_set_tuning(b"fault_alloc_after", -1)
            assert rc == self._lib.CBH_E_NOMEM and _tuning(L, b"fault_fired") == fired0 + 1, rc
            L.cbh_clear_error()
        elif name == "remove":
            ix.remove(a["ids"].tolist())
        elif name == "slice":
            self.idx.append(ix.slice(a["ids"].tolist()))
        else:
            raise ValueError(op)

    def search(self, op, a):
        name, ix = op[0], self.idx[op[1]]
        p = self.gpu.SearchParams(cvThresh=op[3] if name in ("find", "find_by_id") else op[4] if name == "find_batch" else 25)
        if name == "knn":
            r, d, c = ix.knn(a["q"], op[4], op[5])
            return V._cut(r, d, c, op[4])
        if name == "knn_media":
            r, d, media, c = ix.knn_media(a["q"], op[4], op[5])
            return [row + [media[q, :len(row[1])].tolist()] for q, row in enumerate(V._cut(r, d, c, op[4]))]
        if name == "radius_match":
            got, first = ix.radius_match(a["q"], op[4])
            assert (got[:, 0] == np.repeat(np.arange(len(a["q"])), np.diff(first))).all()
            return [list(zip(got[first[q]:first[q + 1], 1].tolist(), got[first[q]:first[q + 1], 2].tolist())) for q in range(len(a["q"]))]
        if name == "find":
            return [(x.mediaId, x.score) for x in ix.find(_M(a["id"], a["d"]), p)]
        if name == "find_by_id":
            return [(x.mediaId, x.score) for x in ix.find(_M(a["id"], None), p)]
        if name == "find_batch":
            return [[(x.mediaId, x.score) for x in r] for r in ix.find_batch([_M(mid, d) for mid, d in a["needles"]], p)]
        if name == "descriptors":
            return ix.descriptorsForMediaId(a["id"])
        raise ValueError(op)


class RealVideo:
    """the device side of a "video" sequence: one DctVideoIndex per handle number"""

    sharded = False

    def __init__(self, gpu, shards, radix):
        from types import SimpleNamespace

        from cbird_amd import _lib
        from cbird_amd.video import DctVideoIndex, VideoSearchParams

        self._lib, self.L, self.cls, self.ns, self.radix = _lib, _lib.lib(), DctVideoIndex, SimpleNamespace, radix
        self.params = lambda skip: VideoSearchParams(dctThresh=W.THRESH, skipFrames=skip, minFramesMatched=W.VFM,
                                                     minFramesNear=W.VFN, videoRadix=radix, filterSelf=True)
        self.idx = [DctVideoIndex(radix_compat=radix > 0, shards=shards) if shards else DctVideoIndex(radix_compat=radix > 0)]

    def close(self):
        self.idx.clear()
        gc.collect()

    def mutate(self, op, a):
        L, ix = self.L, self.idx[op[1]]
        if op[0] in ("add", "add_dull", "add_again"):
            for mid, (f, h) in zip(a["ids"].tolist(), a["clips"]):
                f, h = np.ascontiguousarray(f, np.int32), _u64(h)
                self._lib.check(L.cbh_vidx_add_video(ix.handle, mid, _p(f), _p(h), len(f)), "add_video")
        elif op[0] == "remove":
            ids = _u32(a["ids"])
            self._lib.check(L.cbh_vidx_remove(ix.handle, _p(ids), len(ids)), "remove")
        elif op[0] == "slice":
            ids = _u32(a["ids"])
            h = L.cbh_vidx_slice(ix.handle, _p(ids), len(ids))
            assert h, L.cbh_last_error()
            self.idx.append(self.cls(radix_compat=self.radix > 0, _handle=h))
        else:
            raise ValueError(op)

    def search(self, op, a):
        ix, p = self.idx[op[1]], self.params(op[-1])
        tup = lambda ms: [(x.mediaId, x.score, x.range.srcIn, x.range.dstIn, x.range.len) for x in ms]  # noqa: E731
        vid = lambda n: self.ns(id=n[0], path="", videoIndex=self.ns(frames=n[1], hashes=n[2], isEmpty=lambda: len(n[1]) == 0))  # noqa: E731
        img = lambda n: self.ns(id=0, path="", dctHash=n[0], matchRange=self.ns(dstIn=n[1]))  # noqa: E731
        if op[0] == "find_video":
            return tup(ix.findVideo(vid(a["needle"]), p))
        if op[0] == "find_videos_batch":
            return [tup(r) for r in ix.find_videos_batch([vid(n) for n in a["needles"]], p)]
        if op[0] == "find_frame":
            return tup(ix.findFrame(img(a["needle"]), p))
        if op[0] == "find_frames_batch":
            return [tup(r) for r in ix.find_frames_batch([img(n) for n in a["needles"]], p)]
        if op[0] == "entries":
            return ix.entries(op[2])
        if op[0] in ("coverage", "segments"):
            import video_coverage_rules as VR
            import video_segments_rules as SR

            call = ix.coverage if op[0] == "coverage" else lambda pairs, p: ix.segments(pairs, p, tol=W.TOL, max_segments=W.MAX_SEGMENTS)
            out = []
            for r in call(a["pairs"], p):
                if op[0] == "coverage":
                    out.append([[getattr(r, k) for k in VR.FIELDS], r.frames, r.dst_frames, r.distances])
                else:
                    out.append([[getattr(r, k) for k in SR.SUMMARY_FIELDS],
                                [[getattr(g, k) for k in SR.SEGMENT_FIELDS] for g in r.segments], r.frames, r.dst_frames,
                                r.distances, r.segment_of])
            try:  # a pair that names an id the handle does not hold refuses the whole call
                call(a["pairs"] + [a["bad"]], p)
                out.append("accepted")
            except self._lib.CbhError as e:
                out.append("INVAL" if e.code == self._lib.CBH_E_INVAL else e.code)
                self.L.cbh_clear_error()
            return out
        raise ValueError(op)


def run_video(gpu, name, ops, shards, radix):
    """as run(), with the video index's own counters: memoryUsage() is 0 right after a mutation and 14 bytes per entry
    of the structure the next search builds; entries(skip) is the mirror's count under the BUILT skip"""
    from cbird_amd import _lib
    from oracle import VideoOracle

    L, vorc = _lib.lib(), VideoOracle()
    live0 = _tuning(L, b"arena_live_bytes")
    world, real = W.World(), RealVideo(gpu, shards, radix)
    step = -1
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for step, op in enumerate(ops):
                a = W.resolve(world, op)
                ix = real.idx[op[1]]
                if W.is_search(op):
                    want, entries = W.expect(world, op, a, vorc, radix)
                    got = real.search(op, a)
                    assert S.canon(got) == S.canon(want), f"{op}: {_first_difference(S.canon(got), S.canon(want))}"
                    if entries is not None:
                        assert ix.memoryUsage() == 14 * entries, (op, ix.memoryUsage(), entries)
                else:
                    real.mutate(op, a)
                    W.apply_mutation(world, op, a)
                    if op[0] != "slice":
                        assert ix.memoryUsage() == 0, op
                    else:
                        assert real.idx[-1].memoryUsage() == 0, op
                assert ix.count() == world.handles[op[1]].count(), op
    except Exception as e:
        raise AssertionError(f"{type(e).__name__}: {e}\n" + S.paste("video", name, ops[:step + 1])) from e
    finally:
        real.close()
    assert _tuning(L, b"arena_live_bytes") == live0, name


def _first_difference(got, want):
    if type(got) is not type(want) or not isinstance(got, list):
        return f"got {got!r}, want {want!r}"
    if len(got) != len(want):
        return f"length {len(got)}, want {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return f"[{i}] " + _first_difference(g, w)
    return "equal"


TREE_PROBE = S.gen_hashes(99, 32)


def run(gpu, orc, kind, name, ops, joined=False):
    """`ops` on the device and on the mirror; -> facts about the run for the counter checks"""
    from cbird_amd import _lib

    L = _lib.lib()
    live0 = _tuning(L, b"arena_live_bytes")
    if kind in V.KINDS:
        from oracle import CvOracle

        mod, world, real, orc = V, V.World(kind), RealCv(gpu, kind), CvOracle()
    else:
        mod, world, real = S, S.World(kind), RealColor(gpu) if kind == "color" else Real(gpu, kind)
    joins = {"searches": 0, "mutations_after": 0, "pending": set(), "scan_joins": 0, "rescans": 0}
    rule, rescans_seen = S.RescanRule(), 0
    counted = kind in ("dcthash", "fdct", "fdct_tree")  # (the kinds whose searches go through scan_all)
    stats = None
    step = -1
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # ("no hash for needle", "empty/null tree": the reference's qWarning)
            for step, op in enumerate(ops):
                a = mod.resolve(world, op)
                m = world.handles[op[1]]
                if mod.is_search(op):
                    want = S.canon(mod.expect(world, op, a, orc))
                    j0 = _tuning(L, b"scan_joins")
                    a0 = real.scan_attempts(real.idx[op[1]]) if counted else 0
                    got = S.canon(real.search(op, a))
                    assert got == want, f"{op}: {_first_difference(got, want)}"
                    if counted and op[0] == "find_batch" and m.count():
                        # scan_all's attempts: one, and more only where the block was too small -- seen on the device
                        again = real.scan_attempts(real.idx[op[1]]) - a0 - (0 if real.sharded else 1)
                        assert 0 <= again <= (2 * real.shards if real.sharded else 2), (op, again)
                        if m.rec_cap == S.REC_CAP_DEFAULT:
                            assert again == 0, (op, again)
                        elif m.rec_cap == S.SMALL_REC_CAP and rule.must(op, m, S._records(kind, m, a, op[4]), real.shards):
                            assert again >= 1, f"{op}: more records than the block of 1024 holds, and no second scan"
                            rescans_seen += 1
                        if joined and op[4] <= 8:  # every attempt of a joined search is one join, and nothing else is
                            dj = _tuning(L, b"scan_joins") - j0
                            assert dj == 1 + again, (op, dj, again)
                            joins["searches"] += 1
                            joins["scan_joins"] += dj
                            joins["rescans"] += again
                            joins["pending"].add(op[1])
                    if counted:
                        rule.search(op, m)
                else:
                    real.mutate(op, a)
                    rule.mutation(op)
                    changed = mod.apply_mutation(world, op, a)
                    if changed and op[1] in joins["pending"]:
                        joins["pending"].discard(op[1])
                        joins["mutations_after"] += 1
                    if changed and kind == "fdct_tree":
                        got, want = real._tree_masks(real.idx[op[1]], TREE_PROBE), orc.htree_leaf_masks(m.h, TREE_PROBE)
                        assert (got == want).all(), f"{op}: the tree's shape after the mutation"
                assert real.idx[op[1]].count() == world.handles[op[1]].count(), op
        if joined:
            st = [ix.join_stats() for ix in real.idx]
            stats = {"drops": sum(s.drops for s in st), "builds": sum(s.builds for s in st), "hits": sum(s.hits for s in st), **joins}
        if counted and name != "hand_dcthash_tree" and (not real.sharded or real.shards == 5):
            # the sequence holds a result that a block of 1024 records cannot take, and the handle was seen to scan twice
            assert rescans_seen >= 1, "no rescan was observed"
    except Exception as e:
        raise AssertionError(f"{type(e).__name__}: {e}\n" + S.paste(kind, name, ops[:step + 1])) from e
    finally:
        L.cbh_set_tuning(b"fault_alloc_after", -1)
        real.close()
    # no device memory is kept: the handles are gone, and so is every arena block their calls took
    assert _tuning(L, b"arena_live_bytes") == live0, (kind, name)
    return stats


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("dcthash"))
def test_dcthash_index_sequences(gpu, orc, index_shape, name):
    run(gpu, orc, "dcthash", name, dict(cases("dcthash"))[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("dcthash"))
def test_dcthash_index_sequences_on_the_resident_join(gpu, orc, name):
    """"scan_mfma" 4 with "join_resident" 1: every find_batch at thresholds <= 8 without masks is a bucketed join on tables
    the handle keeps -- thresholds 4, 5 and 8 are its three kernels and two plan sizes.  A table survives exactly the
    calls between two mutations: `drops` counts the mutations that found one, `hits` the searches that did."""
    from cbird_amd import _lib

    L = _lib.lib()
    assert L.cbh_set_tuning(b"scan_mfma", 4) == 0 and L.cbh_set_tuning(b"join_resident", 1) == 0
    try:
        st = run(gpu, orc, "dcthash", name, dict(cases("dcthash"))[name], joined=True)
    finally:
        L.cbh_set_tuning(b"scan_mfma", 1)
        L.cbh_set_tuning(b"join_resident", 0)
    print(name, st)
    if name == "hand_dcthash_tree":  # (masked searches only: the join takes none of them)
        assert st["searches"] == 0
        return
    assert st["searches"] > 0
    assert st["drops"] >= st["mutations_after"], st
    assert st["builds"] >= st["drops"] and st["hits"] >= 1, st
    # "scan_joins" moved by one per joined search, and by one more per second scan of a search whose block was too small
    assert st["scan_joins"] == st["searches"] + st["rescans"] and st["rescans"] >= 1, st


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("fdct"))
@pytest.mark.parametrize("kind", ["fdct", "fdct_tree"])
def test_dctfeatures_index_sequences(gpu, orc, index_shape, reduce_path, kind, name):
    run(gpu, orc, kind, name.replace("hand_fdct", "hand_" + kind), dict(cases(kind))[name.replace("hand_fdct", "hand_" + kind)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("color"))
def test_color_index_sequences(gpu, orc, name):
    """hand_color holds the regression "a refused add leaves nothing behind": before the fix cbh_color_add appended the
    host copies of the refused entries first, and the next add uploaded them in place of its own"""
    run(gpu, orc, "color", name, dict(cases("color"))[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("cv"))
@pytest.mark.parametrize("kind", ["cv", "cv_sharded"])
def test_cvfeatures_index_sequences(gpu, kind, name):
    """plain: 65 000 rows, then across the first block of 65 536; shards=(1, 3): 84 000 rows in adds of 6 000, every shard
    the current one twice, the per-shard segment tables rebuilt whenever rows arrived"""
    name = name.replace("hand_cv", "hand_" + kind)
    run(gpu, None, kind, name, dict(cases(kind))[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("video"))
@pytest.mark.parametrize("radix", [0, W.RADIX])
@pytest.mark.parametrize("shards", [None, (1, 5)], ids=["one", "shards5"])
def test_video_index_sequences(gpu, reduce_path, shards, radix, name):
    """the structure is built by the first search after a mutation with that search's skipFrames and kept until the next
    mutation; radix 10 is the RadixMap-compatible search (DctVideoIndex(radix_compat=True), -p.vradix 10)"""
    run_video(gpu, name, dict(cases("video"))[name], shards, radix)
