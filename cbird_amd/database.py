"""The caller contract around Index::find: Database::searchIndex and the -similar driver
(src/database.cpp:1209-1278, 1280-1466, 1691-1757), restated for in-memory media lists.

Only the parts that shape the search RESULT are here (threshold escalation, ordering, self filter, maxMatches
cut, the path / inPath and filterParent filters, minMatches acceptance, duplicate-group filter, mergeGroups /
expandGroups); SQL, negative-match lists and weeds are other tables of the database (out of
scope).

`similar()` has two routes with identical results: the reference's shape (one find() per needle, Python code
below) and, for DctHashIndex, the whole job behind the C-ABI (cbh_search_index_batch + cbh_filter_groups).
The test suite holds both against a third, independent C restatement of the same reference lines
(tests/test_database.py).
"""
from __future__ import annotations

import copy
import warnings

from .index import Match, SearchParams


def _sorted_matches(matches):
    """std::sort(matches) by score (index.h:284, unstable in the reference); ties fixed to ascending
    mediaId -- SURVEY.md section 7, hard part 2."""
    return sorted(matches, key=lambda m: (m.score, m.mediaId))


def _escalate(params: SearchParams, tmp: SearchParams) -> bool:
    """one step of the maxThresh loop (database.cpp:1706-1722); False = stop"""
    if params.algo in (SearchParams.AlgoDCT, SearchParams.AlgoDCTFeatures, SearchParams.AlgoVideo):
        tmp.dctThresh += 1
        return tmp.dctThresh <= params.maxThresh
    if params.algo == SearchParams.AlgoCVFeatures:
        tmp.cvThresh += 5
        return tmp.cvThresh <= params.maxThresh
    if params.algo == SearchParams.AlgoColor:
        return False
    warnings.warn("maxThresh: unsupported algorithm")
    return False


def _group_from_matches(needle, matches, params, id_map):
    group = []
    for match in _sorted_matches(matches):
        if params.filterSelf and int(match.mediaId) == needle.id:
            continue
        if len(group) >= params.maxMatches:
            break
        media = id_map.get(int(match.mediaId))
        if media is not None and media.isValid():
            media = copy.copy(media)
            media.score = match.score
            media.matchRange = match.range
            group.append(media)
        else:
            warnings.warn(f"no media with id: {int(match.mediaId)}, index could be stale or corrupt")
    return group


def search_index(index, needle, params: SearchParams, id_map: dict):
    """Database::searchIndex (database.cpp:1691-1757)"""
    matches = index.find(needle, params)
    if params.maxThresh > 0:
        tmp = copy.copy(params)
        while len(matches) <= params.minMatches:
            if not _escalate(params, tmp):
                break
            matches = index.find(needle, tmp)
    return _group_from_matches(needle, matches, params, id_map)


def search_index_batch(index, needles, params: SearchParams, id_map: dict):
    """Database::searchIndex for a needle batch behind the C-ABI (cbh_*_search_index_batch, searchbatch.hip /
    search.hip): one batched find per threshold level instead of one find per needle and level.  Returns what
    [search_index(index, m, params, id_map) for m in needles] returns."""
    import ctypes as C

    import numpy as np

    from . import _lib
    from .index import DctFeaturesIndex, DctHashIndex, MatchRange

    L = _lib.lib()
    needles = list(needles)
    n, k = len(needles), int(params.maxMatches)
    nid = np.ascontiguousarray([m.id for m in needles], np.uint32)
    valid = np.unique(np.array(sorted(id_map), np.uint32))
    counts = np.zeros(max(n, 1), np.uint32)
    vargs = (valid.ctypes.data, len(valid))
    fs = int(bool(params.filterSelf))
    cls = type(index).__name__
    if isinstance(index, DctHashIndex):
        mi, ms, mc = index.search_index_batch([m.dctHash for m in needles], nid, params, valid_ids=valid)
        rows = [[(int(mi[j, t]), int(ms[j, t]), None) for t in range(int(mc[j]))] for j in range(n)]
    elif isinstance(index, DctFeaturesIndex):
        hs = [np.asarray(list(getattr(m, "keyPointHashes", []) or []), np.uint64) for m in needles]
        hs = [h if len(h) or m.id <= 0 else index.hashesForId(m.id) for h, m in zip(hs, needles)]  # (:270-276)
        offs = np.zeros(n + 1, np.uint64)
        np.cumsum([len(h) for h in hs], out=offs[1:])
        allh = np.ascontiguousarray(np.concatenate(hs) if n else np.zeros(0, np.uint64), np.uint64)
        out = np.zeros((max(n, 1), max(k, 1), 2), np.uint32)
        _lib.check(L.cbh_fdct_search_index_batch(index.handle, allh.ctypes.data, offs.ctypes.data, nid.ctypes.data, n,
                                                 int(params.dctThresh), int(params.maxThresh), int(index.tree_compat),
                                                 int(params.minMatches), k, fs, *vargs, out.ctypes.data,
                                                 counts.ctypes.data), "fdct_search_index_batch")
        sc = out[..., 1].view(np.int32)
        rows = [[(int(out[j, t, 0]), int(sc[j, t]), None) for t in range(int(counts[j]))] for j in range(n)]
    elif cls == "CvFeaturesIndex":
        ds = [index._rows(m.keyPointDescriptors) for m in needles]
        offs = np.zeros(n + 1, np.uint64)
        np.cumsum([len(d) for d in ds], out=offs[1:])
        allr = np.ascontiguousarray(np.concatenate(ds) if n else np.zeros((0, 32), np.uint8))
        out = np.zeros((max(n, 1), max(k, 1), 2), np.uint32)
        _lib.check(L.cbh_idx256_search_index_batch(index.handle, allr.ctypes.data, offs.ctypes.data, nid.ctypes.data, n,
                                                   int(params.cvThresh), int(params.maxThresh), index.KNN,
                                                   int(params.minMatches), k, fs, *vargs, out.ctypes.data,
                                                   counts.ctypes.data), "idx256_search_index_batch")
        sc = out[..., 1].view(np.int32)
        rows = [[(int(out[j, t, 0]), int(sc[j, t]), None) for t in range(int(counts[j]))] for j in range(n)]
    elif cls == "ColorDescIndex":
        from .colordesc import COLOR_DTYPE

        d = np.ascontiguousarray(np.asarray([m.colorDescriptor for m in needles], COLOR_DTYPE).reshape(-1))
        out = np.zeros((max(n, 1), max(k, 1), 2), np.uint32)
        _lib.check(L.cbh_color_search_index_batch(index._h, d.ctypes.data, nid.ctypes.data, n, k, fs, *vargs,
                                                  out.ctypes.data, counts.ctypes.data), "color_search_index_batch")
        sc = out[..., 1].view(np.int32)
        rows = [[(int(out[j, t, 0]), int(sc[j, t]), None) for t in range(int(counts[j]))] for j in range(n)]
    elif cls == "DctVideoIndex":
        index._apply_radix(params)
        # DctVideoIndex::find (dctvideoindex.cpp:282-289): a needle with a video index is a video needle (findVideo), any
        # other an image needle (findFrame); each part goes to its own entry point, the rows come back in needle order
        is_video = [getattr(m, "videoIndex", None) is not None for m in needles]
        rows = [None] * n

        def take(part, out, cnt):
            for i, j in enumerate(part):
                rows[j] = [(out[i * k + t].id, out[i * k + t].score,
                            MatchRange(out[i * k + t].src_in, out[i * k + t].dst_in, out[i * k + t].len))
                           for t in range(int(cnt[i]))]

        part = [j for j in range(n) if is_video[j]]
        if part:
            vn = [needles[j] for j in part]
            f = np.concatenate([np.asarray(m.videoIndex.frames, np.int32) for m in vn])
            h = np.concatenate([np.asarray(m.videoIndex.hashes, np.uint64) for m in vn])
            offs = np.zeros(len(vn) + 1, np.uint64)
            np.cumsum([len(m.videoIndex.frames) for m in vn], out=offs[1:])
            pid = np.ascontiguousarray(nid[part])
            cnt = np.zeros(len(vn), np.uint32)
            out = (_lib.cbh_vmatch * max(1, len(vn) * max(k, 1)))()
            _lib.check(L.cbh_vidx_search_index_batch(index._h, f.ctypes.data, h.ctypes.data, offs.ctypes.data,
                                                     pid.ctypes.data, len(vn), int(params.dctThresh), int(params.maxThresh),
                                                     int(params.skipFrames), int(params.minFramesMatched),
                                                     int(params.minFramesNear), int(params.minMatches), k, fs, *vargs, out,
                                                     cnt.ctypes.data), "vidx_search_index_batch")
            take(part, out, cnt)
        part = [j for j in range(n) if not is_video[j]]
        if part:
            h = np.ascontiguousarray([int(needles[j].dctHash) for j in part], np.uint64)
            si = np.ascontiguousarray([int(getattr(needles[j], "matchRange", MatchRange()).dstIn) for j in part], np.int32)
            pid = np.ascontiguousarray(nid[part])
            cnt = np.zeros(len(part), np.uint32)
            out = (_lib.cbh_vmatch * max(1, len(part) * max(k, 1)))()
            _lib.check(L.cbh_vidx_search_index_frames_batch(index._h, h.ctypes.data, si.ctypes.data, pid.ctypes.data,
                                                            len(part), int(params.dctThresh), int(params.maxThresh),
                                                            int(params.skipFrames), int(params.minMatches), k, fs, *vargs,
                                                            out, cnt.ctypes.data), "vidx_search_index_frames_batch")
            take(part, out, cnt)
    else:
        raise TypeError(f"search_index_batch: unsupported index {cls}")
    groups = []
    for r in rows:
        g = []
        for mid, score, rng in r:
            media = copy.copy(id_map[mid])
            media.score = score
            if rng is not None:
                media.matchRange = rng
            g.append(media)
        groups.append(g)
    return groups


# Media::parseArchivePath (src/media.cpp:1039-1043, 1083-1099): "<zip>:<member>" virtual paths
_ZIP_MARKERS = (".zip:", ".ZIP:", ".cbz:", ".CBZ:", ".epub:", ".EPUB:", ".odt:", ".ODT:", ".ods:", ".ODS:", ".odp:", ".ODP:",
                ".docx:", ".DOCX:", ".pptx:", ".PPTX:", ".xlsx:", ".XLSX:", ".xps:", ".XPS")


def parse_archive_path(path: str):
    """(parent, child) of a zip-member path, None for a plain file"""
    end = path.rfind(":")
    while end > 1:
        for marker in _ZIP_MARKERS:
            start = end - len(marker) + 1
            if start < 0:
                continue
            if path[start:start + len(marker)] == marker:
                cut = start + len(marker)
                return path[:cut - 1], path[cut:]
        end = path.rfind(":", 0, end)  # lastIndexOf(':', end - 1)
    return None


def dir_path(path: str) -> str:
    """Media::dirPath (src/media.cpp:198-208): the archive for a zip member, else everything before the last '/'"""
    a = parse_archive_path(path)
    if a:
        return a[0]
    i = path.rfind("/")
    return "" if i < 0 else path[:i]


def filter_match(params, match, db_path: str = "") -> bool:
    """Database::filterMatch (src/database.cpp:1209-1248) on one group [needle, match...], in place; True = drop it.
    negativeMatch and the weed marks need other tables and are not here."""
    if params.path != "" and len(match) > 1:
        prefix = params.path
        if not prefix.startswith(db_path):
            prefix = db_path + "/" + params.path
        match[:] = [match[0]] + [m for m in match[1:] if (not params.inPath) ^ m.path.startswith(prefix)]
    if params.filterParent and len(match) > 1:
        parent = dir_path(match[0].path)
        match[:] = [match[0]] + [m for m in match[1:] if dir_path(m.path) != parent]
    return not len(match) > params.minMatches


def merge_group_list(groups):
    """Media::mergeGroupList (src/media.cpp:300-324); Media equality is by path (media.h:237); a merged group is
    ordered by score (Media::operator<), equal scores by path"""
    for i in range(len(groups)):
        for j in range(len(groups)):
            if i == j:
                continue
            a, b = groups[i], groups[j]
            if b and any(m.path == b[0].path for m in a):
                for m in b[1:]:
                    if not any(x.path == m.path for x in a):
                        a.append(m)
                del b[:]
                a.sort(key=lambda m: (m.score, m.path))
    return [g for g in groups if g]


def expand_group_list(groups):
    """Media::expandGroupList (src/media.cpp:326-331)"""
    return [[g[0], m] for g in groups for m in g[1:]]


def filter_matches(params, groups):
    """Database::filterMatches (src/database.cpp:1250-1278)"""
    if getattr(params, "filterGroups", True):
        groups = sorted(groups, key=lambda g: g[0].path)  # stable, like Media::sortGroupList
        seen, out = set(), []
        for g in groups:
            key = tuple(sorted(m.path for m in g))
            if key not in seen:
                seen.add(key)
                out.append(g)
        groups = out
    if getattr(params, "mergeGroups", 0):
        groups = merge_group_list(groups)
    elif getattr(params, "expandGroups", False):
        groups = expand_group_list(groups)
    return groups


def filter_results(params, results, db_path: str = ""):
    """the tail of Database::similar (:1446-1463) on [needle, match...] lists: filterMatch per group, filterMatches,
    order by the first member's path"""
    kept = []
    for g in results:
        if len(g) <= 1:  # a needle without a result is no group (:1409)
            continue
        g = list(g)
        if not filter_match(params, g, db_path):
            kept.append(g)
    return sorted(filter_matches(params, kept), key=lambda g: g[0].path)


def media_attributes(media, params, db_path: str = ""):
    """what cbh_filter_groups_ex takes instead of strings: for every media (ascending id) the rank of its path among
    all sorted paths, a number per distinct dirPath(), and whether the path lies under params.path"""
    import numpy as np

    media = sorted(media, key=lambda m: m.id)
    ids = np.array([m.id for m in media], np.uint32)
    order = sorted(range(len(media)), key=lambda i: media[i].path)
    rank = np.zeros(len(media), np.uint32)
    rank[order] = np.arange(len(media), dtype=np.uint32)
    dirs = {}
    dir_id = np.array([dirs.setdefault(dir_path(m.path), len(dirs)) for m in media], np.uint32)
    prefix = params.path
    if prefix != "" and not prefix.startswith(db_path):
        prefix = db_path + "/" + params.path
    under = np.array([1 if (prefix != "" and m.path.startswith(prefix)) else 0 for m in media], np.uint8)
    return ids, rank, dir_id, under


def filter_groups_c_abi(params, needle_ids, pairs, counts, media, db_path: str = ""):
    """cbh_filter_groups_ex on per-needle results (pairs[nq, k, 2] = (id, score), counts[nq]); returns the groups as
    lists of (mediaId, score), the needle first with score -1"""
    import ctypes as C

    import numpy as np

    from . import _lib

    ids, rank, dir_id, under = media_attributes(media, params, db_path)
    needle_ids = np.ascontiguousarray(needle_ids, np.uint32)
    pairs = np.ascontiguousarray(pairs, np.uint32)
    counts = np.ascontiguousarray(counts, np.uint32)
    nq, k = len(needle_ids), pairs.shape[1] if pairs.ndim == 3 else 1
    fp = _lib.cbh_filter_params(int(params.minMatches), int(bool(getattr(params, "filterGroups", True))),
                                int(bool(params.filterParent)), 0 if params.path == "" else (1 if params.inPath else 2),
                                int(params.mergeGroups), int(bool(params.expandGroups)))
    cap_g = cap_m = 0
    while True:
        first = np.zeros(cap_g + 1, np.uint64)
        members = np.zeros((max(cap_m, 1), 2), np.uint32)
        ng, nm = C.c_size_t(0), C.c_size_t(0)
        rc = _lib.lib().cbh_filter_groups_ex(needle_ids.ctypes.data, pairs.ctypes.data, counts.ctypes.data, nq, k,
                                             C.byref(fp), ids.ctypes.data, rank.ctypes.data, dir_id.ctypes.data,
                                             under.ctypes.data, len(ids), first.ctypes.data, cap_g, members.ctypes.data,
                                             cap_m, C.byref(ng), C.byref(nm))
        if rc == _lib.CBH_E_OVERFLOW:
            cap_g, cap_m = ng.value, nm.value
            continue
        _lib.check(rc, "filter_groups_ex")
        sc = members[:, 1].view(np.int32)
        return [[(int(members[t, 0]), int(sc[t])) for t in range(int(first[g]), int(first[g + 1]))]
                for g in range(ng.value)]


def similar_to(index, needle, params: SearchParams, id_map: dict, db_path: str = ""):
    """Database::similarTo (src/database.cpp:1468-1536; the inSet slice is not here): searchIndex, then filterMatch on
    [needle, match...] -- which clears the list when it keeps no more than minMatches entries -- and the needle dropped"""
    return _filtered(needle, search_index(index, needle, params, id_map), params, db_path)


def _filtered(needle, group, params, db_path):
    """similarTo's tail (:1494-1502) on searchIndex's result"""
    result = [needle] + list(group)
    if filter_match(params, result, db_path):
        result = []
    return result[1:]


_MIRROR_FLAGS = (SearchParams.MirrorHorizontal, SearchParams.MirrorVertical, SearchParams.MirrorBoth)
_TURN_FLAGS = (SearchParams.TurnRight, SearchParams.TurnLeft, SearchParams.Transpose, SearchParams.AntiTranspose)


def mirrored(needle, view):
    """Engine::mirrored (src/engine.cpp:357-365): the Media processImage makes of the reflected image, here from its
    IndexResult (scanner.process_images_views).  processImage builds a new Media (scanner.cpp:864) with the needle's path
    and no database id -- Media::setDefaults sets id 0 (media.cpp:105) -- so searchIndex's filterSelf (database.cpp:1736)
    never drops the needle's own id from a mirrored list, while the path filters see the needle's path."""
    m = copy.copy(needle)
    m.id = 0
    m.dctHash = int(view.dctHash)
    m.keyPointHashes = [int(x) for x in view.keyPointHashes]
    m.keyPointDescriptors = view.keyPointDescriptors
    m.colorDescriptor = view.colorDescriptor
    return m


def _needle_views(needle, params, views):
    """the needle and its reflections in the order Engine::query searches them (engine.cpp:429-436), then its quarter
    turns and transposes (params.turnMask) in flag order"""
    out = [needle]
    for name, flags in (("mirrorMask", _MIRROR_FLAGS), ("turnMask", _TURN_FLAGS)):
        for flag in flags:
            if getattr(params, name, 0) & flag:
                if views is None or views.get(flag) is None:
                    raise ValueError(f"{name} has bit {flag} but no view {flag} of {needle.path!r} was given")
                out.append(mirrored(needle, views[flag]))
    return out


def _compose(lists):
    """matches.append(...) of every list, then std::sort(matches) (engine.cpp:438): Media::operator< (media.h:231-234)
    compares scores only (no match flags are set here) and std::sort is unstable; ties are fixed as in _sorted_matches,
    by mediaId, then by the list (view) they came from.  Duplicates across the lists are kept."""
    tagged = [(m.score, m.id, v, t, m) for v, lst in enumerate(lists) for t, m in enumerate(lst)]
    return [x[-1] for x in sorted(tagged, key=lambda x: x[:4])]


def query(index, needle, params: SearchParams, id_map: dict, views=None, db_path: str = ""):
    """Engine::query from similarTo on (src/engine.cpp:421-438), without the template matcher: similarTo of the needle,
    then for each bit of params.mirrorMask (1 left-right, 2 top-bottom, 4 both, in that order) similarTo of the mirrored
    needle appended, then the same for each bit of params.turnMask (8 / 16 turned right / left, 32 / 64 transposed /
    anti-transposed), each list filtered on its own; the whole sorted by score.  views = the {flag: IndexResult} that
    scanner.process_images_views returned for this needle; a set bit without its view raises ValueError."""
    needles = _needle_views(needle, params, views)
    return _compose([similar_to(index, m, params, id_map, db_path) for m in needles])


def query_batch(index, needles, views, params: SearchParams, id_map: dict, db_path: str = ""):
    """query() for many needles: the needles and all their reflections go through ONE search_index_batch call, the lists
    are then filtered and composed per needle.  views[i] is the {flag: IndexResult} of needles[i] (may be None with
    mirrorMask 0).  Returns [query(index, n, params, id_map, v, db_path) for n, v in zip(needles, views)]."""
    needles = list(needles)
    views = list(views) if views is not None else [None] * len(needles)
    if len(views) != len(needles):
        raise ValueError("one views dict per needle")
    per = [_needle_views(n, params, v) for n, v in zip(needles, views)]
    flat = [m for ms in per for m in ms]
    groups = search_index_batch(index, flat, params, id_map) if flat else []
    out, k = [], 0
    for ms in per:
        out.append(_compose([_filtered(m, groups[k + j], params, db_path) for j, m in enumerate(ms)]))
        k += len(ms)
    return out


def similar(index, haystack, params: SearchParams, batched: bool = True, db_path: str = "", matcher=None):
    """Database::similar for an in-memory haystack (list of Media with unique ids): every item is searched
    as a needle; returns the accepted groups [needle, match1, ...].

    params.templateMatch: every needle's searchIndex result goes through the template matcher (the needle is the template,
    its result the candidates) before the needle is prepended and before filterMatch (src/database.cpp:1418-1421) --
    matcher.match per needle on the batched=False route, ONE matcher.match_groups call for all the groups on the batched
    route; both give the same groups.  The media then need templatematcher.py's ``image`` / ``md5``; matcher=None makes a
    TemplateMatcher().

    batched (DctHashIndex): the whole job behind the C-ABI -- cbh_search_index_batch (scans, escalation and the
    per-needle cut on the device, no per-needle loop here) and cbh_filter_groups_ex (path / parent filters, acceptance,
    duplicate groups, merge / expand, order); this function only turns the surviving rows back into Media objects."""
    if getattr(params, "mirrorMask", 0):
        warnings.warn("reflected images unsupported, use -similar-to")  # database.cpp:1283; ignored, as there
    if getattr(params, "turnMask", 0):
        warnings.warn("turned images unsupported, use -similar-to")  # ignored like mirrorMask
    id_map = {m.id: m for m in haystack}
    tm = bool(getattr(params, "templateMatch", False))
    if tm and matcher is None:
        from .templatematcher import TemplateMatcher

        matcher = TemplateMatcher()
    if batched and hasattr(index, "search_index_batch") and params.algo == SearchParams.AlgoDCT:
        import ctypes as C

        import numpy as np

        from . import _lib

        hay = list(haystack)
        ids = np.array([m.id for m in hay], np.uint32)
        hashes = np.array([m.dctHash for m in hay], np.uint64)
        mi, ms, mc = index.search_index_batch(hashes, ids, params, valid_ids=ids)
        k = int(params.maxMatches)
        pairs = np.zeros((len(hay), max(k, 1), 2), np.uint32)
        pairs[:, :k, 0], pairs[:, :k, 1] = mi, ms.view(np.uint32) if ms.size else ms
        matched = {}  # (needle id, media id) -> the media the matcher scored (its roi / transform are on it)
        if tm:
            mc = np.array(mc, np.uint32)
            tmpls, cands = [], []
            for i, m in enumerate(hay):
                if mc[i]:
                    group = []
                    for t in range(int(mc[i])):
                        media = copy.copy(id_map[int(mi[i, t])])
                        media.score = int(ms[i, t])
                        group.append(media)
                    tmpls.append((i, m)), cands.append(group)
            # the surviving (id, score) rows go back in front of the filters
            for (i, m), group in zip(tmpls, matcher.match_groups([m for _, m in tmpls], cands, params)):
                mc[i] = len(group)
                for t, media in enumerate(group):
                    pairs[i, t, 0] = media.id
                    pairs[i, t, 1] = np.int32(media.score).view(np.uint32)
                    matched[(m.id, media.id)] = media
        # paths enter the C-ABI as per-media attributes (rank of the path, directory number, under-the-prefix flag)
        groups = []
        for g in filter_groups_c_abi(params, ids, pairs, mc, hay, db_path):
            out = []
            for t, (mid, score) in enumerate(g):
                if t == 0 and score == -1:
                    media = id_map[mid]
                else:
                    media = matched.get((g[0][0], mid)) or copy.copy(id_map[mid])
                if not (t == 0 and score == -1):
                    media.score = score
                out.append(media)
            groups.append(out)
        return groups
    results = []
    for m in haystack:
        if params.algo == SearchParams.AlgoDCT and not m.dctHash:
            continue
        group = search_index(index, m, params, id_map)
        if tm and group:
            group = matcher.match(m, group, params)
        results.append([m] + group)
    return filter_results(params, results, db_path)


# ---- clusters: the components of the match graph (no reference counterpart; include/cbird_hip.h) ---------------------
def clusters(index, haystack, params: SearchParams, db_path: str = ""):
    """The partition -similar cannot give: every connected component of the index's match graph at params.dctThresh
    that has more than params.minMatches members (filterMatch's rule, src/database.cpp:1244; never fewer than two), as
    a group of copies of the haystack's Media with score = the distance to the nearest other member.  A group is ordered
    by path and the groups by their first path (:1463).  One device call (DctHashIndex.clusters); a is-similar-to chain
    a ~ c ~ b is ONE group here, where similar(mergeGroups=1) leaves b and c in two.  AlgoDCT only; the path, parent
    and negative-match filters do not apply.  (db_path: accepted for the signature of similar(); paths are compared as
    they are.)"""
    if params.algo != SearchParams.AlgoDCT or not hasattr(index, "clusters"):
        raise ValueError("clusters: only AlgoDCT on a DctHashIndex")
    id_map = {m.id: m for m in haystack}
    groups = []
    for g in index.clusters(int(params.dctThresh), max(2, int(params.minMatches) + 1)):
        out = []
        for mid, score in g:
            if mid not in id_map:
                raise ValueError(f"clusters: the index holds id {mid}, the haystack does not")
            media = copy.copy(id_map[mid])
            media.score = score
            out.append(media)
        groups.append(sorted(out, key=lambda m: m.path))
    return sorted(groups, key=lambda g: g[0].path)


# ---- video coverage: which frames of one clip another contains (no reference counterpart; include/cbird_hip.h) -------
def video_coverage(index, groups, params: SearchParams):
    """For result groups [needle, match1, ...] as similar() returns them for AlgoVideo: needle -> match and match ->
    needle for every member, all in ONE DctVideoIndex.coverage call (summaries only).  Sets on each match
        coverage    the percent of the needle's frames the match contains
        coveredBy   the percent of the match's frames the needle contains
    (whole percents of frame numbers, VideoCoverage.percent) and touches no other attribute; the needle is left alone.
    100 / below 100 reads "the needle is a cut of this match, it is safe to drop the needle".  A member that is no
    video (an image needle of findFrame) is skipped.  Returns the groups."""
    if params.algo != SearchParams.AlgoVideo or not hasattr(index, "coverage"):
        raise ValueError("video_coverage: only AlgoVideo on a DctVideoIndex")
    pairs, where = [], []
    for g in groups:
        if not g or getattr(g[0], "videoIndex", None) is None:
            continue
        for m in g[1:]:
            if getattr(m, "videoIndex", None) is None:
                continue
            where.append(m)
            pairs += [(g[0].id, m.id), (m.id, g[0].id)]
    if pairs:
        res = index.coverage(pairs, params, maps=False)
        for k, m in enumerate(where):
            m.coverage, m.coveredBy = res[2 * k].percent(), res[2 * k + 1].percent()
    return groups


# ---- video segments: at which offsets one clip lies in another (no reference counterpart; include/cbird_hip.h) -------
def video_segments(index, groups, params: SearchParams, tol: int = 15, min_frames=None, max_segments: int = 4):
    """For result groups [needle, match1, ...] as similar() returns them for AlgoVideo: needle -> match for every member,
    all in ONE DctVideoIndex.segments call (no maps).  Sets on each match
        segments    the VideoSegments of the needle inside the match
        aligned     the percent of the needle's frames the match holds at a consistent position (VideoSegments.percent)
    and touches no other attribute -- the match's own range stays findVideo's; segments.match_range() is the precise one.
    A member that is no video (an image needle of findFrame) is skipped.  Returns the groups."""
    if params.algo != SearchParams.AlgoVideo or not hasattr(index, "segments"):
        raise ValueError("video_segments: only AlgoVideo on a DctVideoIndex")
    pairs, where = [], []
    for g in groups:
        if not g or getattr(g[0], "videoIndex", None) is None:
            continue
        for m in g[1:]:
            if getattr(m, "videoIndex", None) is None:
                continue
            where.append(m)
            pairs.append((g[0].id, m.id))
    if pairs:
        res = index.segments(pairs, params, tol=tol, min_frames=min_frames, max_segments=max_segments, maps=False)
        for m, r in zip(where, res):
            m.segments, m.aligned = r, r.percent()
    return groups


# ---- -sort-similar (src/main.cpp:1523-1580) ---------------------------------------------------------------------------
SORT_SIMILAR_LOOK_BEHIND = 5  # `const int lookBehind = 5` (:1530)


def _sort_similar_loop(index, selection, params, db_path):
    """the reference's loop with what exists: a fresh slice of unsorted + needle, one query and one insert per pass"""
    sel = list(selection)
    if not sel:
        return [], 0, 0
    id_map = {m.id: m for m in sel}
    if len(id_map) != len(sel) or 0 in id_map:
        raise ValueError("sort_similar: the selection needs unique non-zero ids")
    ordered = [sel[0]]
    unsorted = {m.id: m for m in sel[1:]}
    queries = not_found = 0
    for _ in range(len(sel) - 1):
        j = 0
        while j < min(SORT_SIMILAR_LOOK_BEHIND, len(ordered)):  # sorted.count() is read again on every pass (:1547)
            needle = ordered[len(ordered) - 1 - j]
            # "set must also contain needle or else we can't search for it" (:1554-1559)
            part = index.slice(list(unsorted) + [needle.id])
            matches = query(part, needle, params, id_map, db_path=db_path)
            if matches:
                hit = id_map[matches[0].id]
                ordered.insert(len(ordered) - j, hit)
                del unsorted[hit.id]
            else:
                not_found += 1
            queries += 1
            j += 1  # no break after an insert: the same needle is asked again one place further back
    return ordered, queries, not_found


def _sort_similar_on_device(index, params) -> bool:
    from .colordesc import ColorDescIndex
    from .index import DctHashIndex

    if (params.mirrorMask or getattr(params, "turnMask", 0) or params.templateMatch or
            not 1 <= int(params.maxMatches) <= 55):
        return False
    if isinstance(index, ColorDescIndex):  # no threshold and no escalation level (src/database.cpp:1707-1718)
        return params.algo == SearchParams.AlgoColor
    return (isinstance(index, DctHashIndex) and params.algo == SearchParams.AlgoDCT and
            0 <= int(params.dctThresh) <= 65 and int(params.maxThresh) <= 65)


def _sort_similar_color(index, selections, params, db_path):
    """the colour route of sort_similar_batch: ONE cbh_color_sort_similar call with the Media's descriptors as needles;
    None when the call refuses the batch (CBH_E_UNSUPPORTED: the loop takes it)"""
    import numpy as np

    from . import _lib
    from .colordesc import COLOR_DTYPE

    flat = [m for s in selections for m in s]
    first = np.zeros(len(selections) + 1, np.uint64)
    np.cumsum([len(s) for s in selections], out=first[1:])
    descs = np.zeros(len(flat), COLOR_DTYPE)
    for k, m in enumerate(flat):
        d = getattr(m, "colorDescriptor", None)
        if d is not None:
            descs[k] = np.asarray(d, COLOR_DTYPE)
    dir_id, under, mode = _path_attributes(flat, params, db_path)
    try:
        got = index.sort_similar([m.id for m in flat], descs, params, first, dir_id, under, mode,
                                 SORT_SIMILAR_LOOK_BEHIND)
    except _lib.CbhError as e:
        if e.code != _lib.CBH_E_UNSUPPORTED:
            raise
        return None
    out = []
    for sel, (order, queries, not_found, _) in zip(selections, got):
        by_id = {m.id: m for m in sel}
        out.append(([by_id[i] for i in order], queries, not_found))
    return out


def _path_attributes(flat, params, db_path):
    """paths as attributes, as in filter_groups_c_abi: a number per distinct dirPath(), under-the-prefix flags, path_mode"""
    import numpy as np

    dir_id = under = None
    if params.filterParent:
        dirs = {}
        dir_id = np.ascontiguousarray([dirs.setdefault(dir_path(m.path), len(dirs)) for m in flat], np.uint32)
    if params.path != "":
        prefix = params.path if params.path.startswith(db_path) else db_path + "/" + params.path
        under = np.ascontiguousarray([1 if m.path.startswith(prefix) else 0 for m in flat], np.uint8)
    return dir_id, under, 0 if params.path == "" else (1 if params.inPath else 2)


def sort_similar_batch(index, selections, params: SearchParams, db_path: str = ""):
    """sort_similar for many selections; DctHashIndex without reflections: ONE cbh_sort_similar call, a workgroup per
    selection (sortsimilar.hip); ColorDescIndex with AlgoColor: ONE cbh_color_sort_similar call -- the score tables
    filled on the device from the index's descriptors and the Media's colorDescriptor as needles, then walked by a
    workgroup per selection (sortsimilar_table.hip); what that call refuses as unsupported (an id twice in the index)
    takes the loop.  Returns [sort_similar(index, s, params, True, db_path) for s in selections]."""
    import ctypes as C

    import numpy as np

    from . import _lib

    if not params.filterSelf:
        raise ValueError("sort_similar: without filterSelf the reference inserts the needle again forever")
    selections = [list(s) for s in selections]
    from .colordesc import ColorDescIndex

    colour = isinstance(index, ColorDescIndex)
    most = _lib.CBH_COLOR_SORT_SIMILAR_MAX if colour else _lib.CBH_SORT_SIMILAR_MAX
    if not (_sort_similar_on_device(index, params) and all(len(s) <= most for s in selections)):
        return [_sort_similar_loop(index, s, params, db_path) for s in selections]
    if colour:
        got = _sort_similar_color(index, selections, params, db_path)
        return got if got is not None else [_sort_similar_loop(index, s, params, db_path) for s in selections]
    flat = [m for s in selections for m in s]
    first = np.zeros(len(selections) + 1, np.uint64)
    np.cumsum([len(s) for s in selections], out=first[1:])
    ids = np.ascontiguousarray([m.id for m in flat], np.uint32)
    hashes = np.ascontiguousarray([int(m.dctHash) for m in flat], np.uint64)
    # the reference searches the index's slice, not the Media list: what the index does not hold is no candidate
    # (every entry with an id, a hash of 0 included: mediaIds() leaves those out, the slice does not)
    L = _lib.lib()
    held = index.download()[1]
    in_index = np.ascontiguousarray(np.isin(ids, held[held != 0]), np.uint8)
    dir_id, under, mode = _path_attributes(flat, params, db_path)
    sp = _lib.cbh_sort_similar_params(int(params.dctThresh), int(params.maxThresh), int(params.minMatches),
                                      int(params.maxMatches), int(bool(params.filterParent)), mode,
                                      SORT_SIMILAR_LOOK_BEHIND)
    out_ids = np.zeros(max(len(flat), 1), np.uint32)
    res = (_lib.cbh_sort_similar_result * max(len(selections), 1))()
    _lib.check(L.cbh_sort_similar(hashes.ctypes.data, ids.ctypes.data, in_index.ctypes.data,
                                  None if dir_id is None else dir_id.ctypes.data,
                                  None if under is None else under.ctypes.data, first.ctypes.data, len(selections),
                                  C.byref(sp), out_ids.ctypes.data, res, getattr(index, "device", 0)), "sort_similar")
    out = []
    for s, sel in enumerate(selections):
        by_id = {m.id: m for m in sel}
        a = int(first[s])
        out.append(([by_id[int(i)] for i in out_ids[a:a + res[s].sorted]], int(res[s].queries), int(res[s].not_found)))
    return out


def sort_similar(index, selection, params: SearchParams, batched: bool = True, db_path: str = ""):
    """-sort-similar (src/main.cpp:1523-1580): the selection ordered so that every item is followed by its nearest
    remaining neighbour -- for each place, up to lookBehind = 5 queries of the last placed items inside the set of
    unplaced ones, a hit inserted behind its needle, no break after a hit, every failing query counted.  Returns
    (sorted media, queries, notFound); items never reached are dropped, as in the reference (:1579).

    batched=False: the reference's shape for any index and any params query() supports -- index.slice() of unsorted +
    needle, query(), insert, once per pass.  batched=True (DctHashIndex, mirrorMask 0): the whole chain in one kernel
    launch, cbh_sort_similar; the Media list stands for the index's slice (items the index does not hold are never
    candidates), so its dctHash values have to be the index's; ColorDescIndex with AlgoColor: cbh_color_sort_similar, the
    candidates' descriptors are the index's and the Media's own are the needles, as in the loop.  Anything else -- the
    keypoint-hash, ORB and video indexes, reflections, the template matcher -- takes the loop.  filterSelf must be set:
    without it the reference inserts the needle again forever (ValueError)."""
    if not params.filterSelf:
        raise ValueError("sort_similar: without filterSelf the reference inserts the needle again forever")
    if batched:
        return sort_similar_batch(index, [selection], params, db_path)[0]
    return _sort_similar_loop(index, selection, params, db_path)


# ---- -merge (src/main.cpp:1582-1652) ------------------------------------------------------------------------------------
MERGE_THRESHOLDS = (12, 1000, 1000, 2 ** 31 - 1)  # "if match.score is >= threshold, use the next algorithm" (:1593-1599)
MERGE_PLACED, MERGE_NO_MATCH, MERGE_MATCH_UNPLACED = 0, 1, 2  # CBH_MERGE_* of include/cbird_hip.h


def _media_ready(needle, algo) -> bool:
    """SearchParams::mediaReady (src/index.cpp:31-52) for algos 0..3"""
    if algo == SearchParams.AlgoDCT:
        return int(needle.dctHash) != 0
    if needle.id != 0:
        return True
    if algo == SearchParams.AlgoDCTFeatures:
        return len(getattr(needle, "keyPointHashes", None) or []) > 0
    if algo == SearchParams.AlgoCVFeatures:
        d = getattr(needle, "keyPointDescriptors", None)
        return d is not None and len(d) > 0
    return getattr(needle, "colorDescriptor", None) is not None


def _merge_indexes(indexes, params):
    if params.algo > SearchParams.AlgoColor:
        raise ValueError("merge: the cascade's threshold table ends at AlgoColor (src/main.cpp:1594-1599)")
    return indexes if isinstance(indexes, dict) else {params.algo: indexes}


def multi_search(indexes, needle, params: SearchParams, id_map: dict, set_ids, db_path: str = ""):
    """the lambda multiSearch of -merge (src/main.cpp:1587-1615) with what exists: maxMatches = 2; from params.algo on,
    query() inside indexes[algo].slice(set_ids) -- the inSet slice of Database::similarTo (src/database.cpp:1475-1486) --
    accepted when there is a match and matches[0].score < MERGE_THRESHOLDS[algo]; otherwise the next algo, up to
    AlgoColor.  An algo without an index, or whose needle is not mediaReady, finds nothing.  Returns (matches, algo), or
    ([], -1) when no stage answered.  indexes maps algo -> index; a bare index stands for {params.algo: index}."""
    indexes = _merge_indexes(indexes, params)
    p = copy.copy(params)
    p.maxMatches = 2
    set_ids = list(set_ids)
    for algo in range(params.algo, SearchParams.AlgoColor + 1):
        p.algo = algo
        index = indexes.get(algo)
        if index is None or not _media_ready(needle, algo):
            continue
        matches = query(index.slice(set_ids), needle, p, id_map, db_path=db_path)
        if matches and matches[0].score < MERGE_THRESHOLDS[algo]:
            return matches, algo
    return [], -1


def _merge_on_device(index, params) -> bool:
    from .index import DctHashIndex

    return (isinstance(index, DctHashIndex) and params.algo == SearchParams.AlgoDCT and not params.templateMatch and
            0 <= int(params.dctThresh) <= 65 and 0 <= int(params.maxThresh) <= 65)


def _merge_find(index, media, n_a, params, db_path):
    """cbh_merge_find for all needles: (match place or -1, score) per needle"""
    import ctypes as C

    import numpy as np

    from . import _lib

    n_b = len(media) - n_a
    ids = np.ascontiguousarray([m.id for m in media], np.uint32)
    hashes = np.ascontiguousarray([int(m.dctHash) for m in media], np.uint64)
    # the reference searches the index's slice, not the Media list: what the index does not hold is no candidate
    held = index.download()[1]
    in_index = np.ascontiguousarray(np.isin(ids, held[held != 0]), np.uint8)
    dir_id, under, mode = _path_attributes(media, params, db_path)
    mp = _lib.cbh_merge_params(int(params.dctThresh), int(params.maxThresh), int(params.minMatches), 2,
                               int(bool(params.filterParent)), mode)
    match = np.zeros(max(n_b, 1), np.uint32)
    score = np.zeros(max(n_b, 1), np.int32)
    _lib.check(_lib.lib().cbh_merge_find(hashes.ctypes.data, ids.ctypes.data, in_index.ctypes.data,
                                         None if dir_id is None else dir_id.ctypes.data,
                                         None if under is None else under.ctypes.data, n_a, n_b, C.byref(mp),
                                         match.ctypes.data, score.ctypes.data, getattr(index, "device", 0)), "merge_find")
    return [(-1 if int(m) == 0xFFFFFFFF else int(m), int(s)) for m, s in zip(match[:n_b], score[:n_b])]


def _merge_place_loop(media, n_a, match):
    """the placement of -merge (src/main.cpp:1628-1650) on a Python list of places"""
    order, status = list(range(n_a)), []
    for k, m in enumerate(match):
        if m < 0:
            status.append(MERGE_NO_MATCH)  # qCritical("no match") (:1631-1634)
            continue
        if m not in order:
            status.append(MERGE_MATCH_UNPLACED)  # the reference's Q_ASSERT (:1640)
            continue
        pos = order.index(m)
        if 0 < pos < len(order) - 1:
            h = int(media[n_a + k].dctHash)
            before = bin(h ^ int(media[order[pos - 1]].dctHash)).count("1")
            after = bin(h ^ int(media[order[pos + 1]].dctHash)).count("1")
            if after < before:
                pos += 1
        order.insert(pos, n_a + k)
        status.append(MERGE_PLACED)
    return order, status


def _merge_place(media, n_a, match):
    """the same through cbh_merge_place"""
    import ctypes as C

    import numpy as np

    from . import _lib

    n_b = len(media) - n_a
    hashes = np.ascontiguousarray([int(m.dctHash) for m in media], np.uint64)
    m32 = np.ascontiguousarray([0xFFFFFFFF if m < 0 else m for m in match] or [0], np.uint32)
    order = np.zeros(max(len(media), 1), np.uint32)
    status = np.zeros(max(n_b, 1), np.uint8)
    n_out = C.c_size_t(0)
    _lib.check(_lib.lib().cbh_merge_place(hashes.ctypes.data, n_a, n_b, m32.ctypes.data, order.ctypes.data,
                                          status.ctypes.data, C.byref(n_out)), "merge_place")
    return [int(i) for i in order[:n_out.value]], [int(s) for s in status[:n_b]]


def merge(indexes, set_a, set_b, params: SearchParams, batched: bool = True, db_path: str = ""):
    """-merge A B (src/main.cpp:1582-1652): every item of set_b put into set_a next to its closest match.  Needle b_k, in
    B's order, is searched with multi_search inside the original A followed by b_0 .. b_k (:1619-1625); a needle with a
    match goes in front of it in the list built so far -- behind it when the match has neighbours on both sides and the
    needle's dctHash is strictly nearer to the one behind (:1643-1648) -- and a needle without one is dropped.  A needle
    whose match is an earlier needle that was dropped aborts the reference (Q_ASSERT, :1640); here it is dropped too,
    with a status of its own.  Returns (merged list of Media, report), report[k] = (status MERGE_*, the algo that
    answered or -1, the score or -1, the match's id or 0) of needle k.

    batched=False: multi_search per needle and the placement in Python -- the reference's shape, for any index.
    batched=True: a DctHashIndex as algo 0 (thresholds within 0..65, no templateMatch) answers ALL needles in one
    cbh_merge_find call (merge.hip; the Media's dctHash stands for the index's, items the index does not hold are never
    candidates); needles it leaves unanswered or answers at a score >= 12 take the later stages through multi_search's
    slice and query; the placement is cbh_merge_place.  Anything else takes multi_search for every needle.
    ValueError: filterSelf off (every needle would find itself), mirrorMask or turnMask set (there are no images here),
    params.algo above AlgoColor, an id 0 or an id twice in A and B."""
    if not params.filterSelf:
        raise ValueError("merge: without filterSelf every needle finds itself in its own set")
    if params.mirrorMask or getattr(params, "turnMask", 0):
        raise ValueError("merge: reflections and turns need the needles' images")
    indexes = _merge_indexes(indexes, params)
    set_a, set_b = list(set_a), list(set_b)
    media, n_a = set_a + set_b, len(set_a)
    id_map = {m.id: m for m in media}
    if len(id_map) != len(media) or 0 in id_map:
        raise ValueError("merge: A and B together need unique non-zero ids")
    ids = [m.id for m in media]
    place_of = {m.id: k for k, m in enumerate(media)}
    found = [None] * len(set_b)  # (place, algo, score)
    rest, later = range(len(set_b)), params
    if batched and set_b and _merge_on_device(indexes.get(SearchParams.AlgoDCT), params):
        first = _merge_find(indexes[SearchParams.AlgoDCT], media, n_a, params, db_path)
        rest = []
        for k, (m, s) in enumerate(first):
            if m >= 0 and s < MERGE_THRESHOLDS[0]:
                found[k] = (m, SearchParams.AlgoDCT, s)
            else:
                rest.append(k)
        later = copy.copy(params)
        later.algo = SearchParams.AlgoDCTFeatures
    for k in rest:
        matches, algo = multi_search(indexes, set_b[k], later, id_map, ids[:n_a + k + 1], db_path)
        if matches:
            found[k] = (place_of[matches[0].id], algo, int(matches[0].score))
    match = [-1 if f is None else f[0] for f in found]
    order, status = (_merge_place if batched else _merge_place_loop)(media, n_a, match)
    report = [(st, -1, -1, 0) if f is None else (st, f[1], f[2], media[f[0]].id) for st, f in zip(status, found)]
    return [media[i] for i in order], report
