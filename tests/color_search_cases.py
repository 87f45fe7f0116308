"""The colour search (cbird_amd/csrc/color.hip) restated in numpy, and the case sets that aim at its edges.

ColorDescriptor::distance (src/cvutil.cpp:682-749): FLT_MAX when a side has no colours or the counts differ by more than
2; otherwise a := the side with more colours (the first argument -- the needle -- on a tie),
score = 1.0f + sum_{i < numA} min_j sqrtf(dl * dl + du * du + dv * dv)  in float, ascending i, colours decompressed as
DescriptorColor::get does (src/cvutil.h:83-87).  np_scores() is that, vectorised, every product and sum rounded to
float32 in the reference's order; the minimum is taken on the squares (sqrtf is monotone and correctly rounded, so the
result is the same bits).  ColorDescIndex::find (src/colordescindex.cpp:250-278) reports int(score) for ids != 0.

np_scores_fused / np_scores_reordered are MUTANTS: the sum of squares as k_color_dist3<.., FMA> forms it (no rounding of
the products), and as dv * dv + du * du + dl * dl.  They exist to prove that a case set can see such a kernel; they are
never what a non-FMA kernel is expected to give.

Case sets
  boundary_pairs        single-colour pairs whose score is an integer or one ulp below one: a last-bit error in the sum of
                        squares moves int(score).  Seed 1, 16 * 10^6 draws: 469 pairs, np_scores_fused moves the int of 31
                        of them, np_scores_reordered of 22.
  boundary_pairs_multi  the same with 8-colour needles against 7-colour entries (a real sum; the needle side is "a"), and
                        mirrored (7 against 8: the entry side is "a").  Seed 3, 10^6 draws: 105 pairs, fused moves 10,
                        reordered moves 9 (the same pairs in either orientation).
  wave_shape_index      numColors in runs, so that whole waves of both kernels stop their colour loop early
  select_cases          the cut of cbh_color_find_batch: window, candidate cap, full sort, k and n at their edges
"""
from collections import namedtuple

import numpy as np

F = np.float32
FLT_MAX = np.finfo(F).max
NC = 32                       # ColorDescriptor::NUM_DESC_COLORS
COLOR_DTYPE = np.dtype([("colors", np.uint16, (NC, 4)), ("numColors", np.uint8), ("_pad", np.uint8)])  # 258 bytes
WIN = 2048                    # kWin: histogram bins above the per-needle minimum score
CAND_CAP = 4096               # kCandCap: candidates per needle the window cut can hold


# ---- the reference and its mutants --------------------------------------------------------------------------------------
def decompress(descs):
    """DescriptorColor::get (cvutil.h:83-87): l, u, v float32 [n, 32] and numColors [n]"""
    d = np.asarray(descs, COLOR_DTYPE).reshape(-1)
    c = d["colors"].astype(F)
    l = c[..., 0] * F(100.0) / F(65535)
    u = c[..., 1] * F(354.0) / F(65535) - F(134.0)
    v = c[..., 2] * F(262.0) / F(65535) - F(140.0)
    return l, u, v, d["numColors"].astype(np.int64)


def sumsq_ref(dl, du, dv):
    return (dl * dl + du * du) + dv * dv


def sumsq_fused(dl, du, dv):
    dl, du, dv = dl.astype(np.float64), du.astype(np.float64), dv.astype(np.float64)
    return (dl * dl + du * du + dv * dv).astype(F)


def sumsq_reordered(dl, du, dv):
    return (dv * dv + du * du) + dl * dl


def _scores(needles, descs, sumsq=sumsq_ref, count_rule=True, swap_sides=False):
    """count_rule=False drops `abs(nn - hn) <= 2`; swap_sides=True sums over the side with FEWER colours (the entry on a
    tie): the two routing mutants of the model test"""
    ql, qu, qv, qn = decompress(needles)
    hl, hu, hv, hn = decompress(descs)
    out = np.full((len(qn), len(hn)), FLT_MAX, F)
    for q in range(len(qn)):
        nn = int(qn[q])
        if nn == 0:
            continue
        ok = hn != 0
        if count_rule:
            ok &= np.abs(hn - nn) <= 2
        idx = np.nonzero(ok)[0]
        if not len(idx):
            continue
        cnt = hn[idx]
        H = int(cnt.max())
        dl = ql[q, :nn, None][None] - hl[idx, None, :H]     # [m, nn, H]
        du = qu[q, :nn, None][None] - hu[idx, None, :H]
        dv = qv[q, :nn, None][None] - hv[idx, None, :H]
        d2 = sumsq(dl, du, dv).astype(F)
        d2 = np.where((np.arange(H)[None, :] < cnt[:, None])[:, None, :], d2, F(np.inf))
        row = np.sqrt(d2.min(axis=2)).astype(F)             # [m, nn]: per needle colour
        col = np.sqrt(d2.min(axis=1)).astype(F)             # [m, H]:  per entry colour
        rs = np.full(len(idx), 1.0, F)
        for p in range(nn):
            rs = (rs + row[:, p]).astype(F)
        cs = np.full(len(idx), 1.0, F)
        for h in range(H):
            cs = np.where(h < cnt, (cs + col[:, h]).astype(F), cs)
        entry_side = nn < cnt
        if swap_sides:
            entry_side = ~entry_side
        out[q, idx] = np.where(entry_side, cs, rs)
    return out


def np_scores(needles, descs):
    """float32 [nq, n]: ColorDescriptor::distance(needle, entry), the reference's operation order"""
    return _scores(needles, descs)


def np_scores_fused(needles, descs):
    return _scores(needles, descs, sumsq_fused)


def np_scores_reordered(needles, descs):
    return _scores(needles, descs, sumsq_reordered)


def int_scores(scores):
    """int(score) as find() reports it; -1 where the reference returns FLT_MAX (no match)"""
    s = np.asarray(scores, F)
    fin = s < FLT_MAX
    return np.where(fin, np.where(fin, s, 0).astype(np.int32), -1).astype(np.int32)


def _on_boundary(s):
    """score an exact integer, or one ulp below one"""
    s = np.asarray(s, F)
    up = np.nextafter(s, F(np.inf))
    return (s == np.floor(s)) | (up == np.floor(up))


def synth_descriptors(n, seed, dup_frac=0.3):
    """(descs, ids): random palettes of 0..32 colours, 5 % without colours, near-duplicates of earlier entries"""
    rng = np.random.default_rng(seed)
    d = np.zeros(n, COLOR_DTYPE)
    num = rng.integers(0, 33, n)
    num[rng.random(n) < 0.05] = 0  # grayscale images: stored with no colours (colordescindex.cpp:73-75)
    for i in range(n):
        if i and rng.random() < dup_frac:  # near-duplicate palette of an earlier entry
            src = int(rng.integers(0, i))
            d[i] = d[src]
            k = int(d[i]["numColors"])
            if k:
                jit = rng.integers(-600, 601, (k, 4))
                d[i]["colors"][:k] = np.clip(d[i]["colors"][:k].astype(np.int64) + jit, 0, 65535)
                drop = int(rng.integers(0, 3))
                d[i]["numColors"] = max(0, k - drop)
        else:
            k = int(num[i])
            d[i]["colors"][:k] = rng.integers(0, 65536, (k, 4))
            d[i]["numColors"] = k
    ids = np.arange(1, n + 1, dtype=np.uint32)
    return d, ids


# ---- boundary sets ------------------------------------------------------------------------------------------------------
BOUNDARY_SEED, BOUNDARY_DRAWS = 1, 16_000_000
MULTI_SEED, MULTI_DRAWS = 3, 1_000_000
_cache = {}


def _pair_scores(a, b, sumsq):
    """scores of pair i = (needle a[i] with A colours, entry b[i] with B colours), A >= B: colours uint16 [m, A|B, 3]"""
    def dec(c):
        c = c.astype(F)
        return (c[..., 0] * F(100.0) / F(65535), c[..., 1] * F(354.0) / F(65535) - F(134.0),
                c[..., 2] * F(262.0) / F(65535) - F(140.0))

    al, au, av = dec(a)
    bl, bu, bv = dec(b)
    d2 = sumsq(al[:, :, None] - bl[:, None, :], au[:, :, None] - bu[:, None, :], av[:, :, None] - bv[:, None, :]).astype(F)
    r = np.sqrt(d2.min(axis=2)).astype(F)
    s = np.full(len(a), 1.0, F)
    for p in range(a.shape[1]):
        s = (s + r[:, p]).astype(F)
    return s


def _draw_boundary(seed, draws, A, B, chunk):
    rng = np.random.default_rng(seed)
    ka, kb = [], []
    for _ in range(draws // chunk):
        a = rng.integers(0, 65536, (chunk, A, 3), dtype=np.uint16)
        b = rng.integers(0, 65536, (chunk, B, 3), dtype=np.uint16)
        keep = _on_boundary(_pair_scores(a, b, sumsq_ref))
        ka.append(a[keep])
        kb.append(b[keep])
    a, b = np.concatenate(ka), np.concatenate(kb)

    def pack(c):
        d = np.zeros(len(c), COLOR_DTYPE)
        d["colors"][:, : c.shape[1], :3] = c
        d["colors"][:, : c.shape[1], 3] = 1
        d["numColors"] = c.shape[1]
        return d

    return pack(a), pack(b)


def diagonal(m):
    m = np.asarray(m)
    return m[np.arange(m.shape[0]), np.arange(m.shape[0])]


def flips(needles, descs, mutant):
    """how many pairs (needle i, entry i) change int(score) under a mutant"""
    ref = int_scores(diagonal(np_scores(needles, descs)))
    return int((int_scores(diagonal(mutant(needles, descs))) != ref).sum())


def boundary_pairs(seed=BOUNDARY_SEED):
    """(needles, descs): pair i = (needles[i], descs[i]), one colour each, scores on an integer boundary"""
    key = ("single", seed)
    if key not in _cache:
        nd, ds = _draw_boundary(seed, BOUNDARY_DRAWS, 1, 1, 1_000_000)
        assert len(nd) >= 300, len(nd)
        assert _on_boundary(diagonal(np_scores(nd, ds))).all()
        assert flips(nd, ds, np_scores_fused) >= 10
        _cache[key] = (nd, ds)
    return _cache[key]


def boundary_pairs_multi(seed=MULTI_SEED, mirrored=False):
    """8-colour needles against 7-colour entries on integer boundaries (the needle side sums: rowacc); mirrored: the
    same pairs the other way round, 7-colour needles against 8-colour entries (the entry side sums: colacc)"""
    key = ("multi", seed)
    if key not in _cache:
        nd, ds = _draw_boundary(seed, MULTI_DRAWS, 8, 7, 50_000)
        assert len(nd) >= 80, len(nd)
        assert _on_boundary(diagonal(np_scores(nd, ds))).all()
        assert flips(nd, ds, np_scores_fused) >= 3
        _cache[key] = (nd, ds)
    nd, ds = _cache[key]
    return (ds, nd) if mirrored else (nd, ds)


# ---- wave shapes --------------------------------------------------------------------------------------------------------
WAVE_COLOURS = (1, 2, 3, 15, 16, 17, 31, 32)
WAVE_SIZES = (1, 2, 255, 256, 257, 511, 512, 513, 1025)
RUN = 130   # entries per run: boundaries at 130 j, never a multiple of 64.  Runs ascend in colour count, so the wave
#             [W j, W j + W) -- W = 64 (k_color_dist3) or 128 (k_color_dist2, two entries per lane) -- holds the tail of
#             run j' - 1 and the head of run j' and has run j''s count as its maximum
_FIRST_RUN = {1: 0, 2: 3, 255: 0, 256: 2, 257: 4, 511: 0, 512: 4, 513: 2, 1025: 0}   # which run an index of n starts with


def wave_runs(n):
    """colour count c of the run every entry 0..n-1 lies in"""
    j = np.minimum(_FIRST_RUN.get(n, 0) + np.arange(n) // RUN, len(WAVE_COLOURS) - 1)
    return np.array(WAVE_COLOURS)[j]


def wave_shape_index(seed, n):
    """(descs, ids, needles, removable): entry i has at most wave_runs(n)[i] colours -- mostly exactly that many, some one
    or two fewer, some none (grayscale), some zeroed as remove() leaves them (id 0, descriptor cleared); needles with
    c - 3 .. c + 3 colours for every run's c (and one without colours); removable: ids inside the runs for remove()"""
    rng = np.random.default_rng([seed, n])
    c = wave_runs(n)
    kind = rng.random(n)
    num = np.where(kind < 0.60, c, np.where(kind < 0.75, c - 1, np.where(kind < 0.85, c - 2, 0)))
    num = np.maximum(num, 0)
    if n > 2:
        first = np.nonzero(np.r_[True, c[1:] != c[:-1]])[0]
        num[first] = c[first]                       # every run holds its full count at least once, at its head ...
        num[np.minimum(first + 70, n - 1)] = c[np.minimum(first + 70, n - 1)]   # ... and in its second dist3 wave
    else:
        num[:] = c
    descs = np.zeros(n, COLOR_DTYPE)
    descs["colors"] = rng.integers(0, 65536, (n, NC, 4))    # colours past numColors stay set: the count is what counts
    descs["numColors"] = num
    ids = np.arange(1, n + 1, dtype=np.uint32)
    if n > 2:
        zeroed = kind >= 0.95
        zeroed[first] = False
        descs[zeroed] = np.zeros((), COLOR_DTYPE)
        ids[zeroed] = 0
    counts = sorted({k for cc in set(c.tolist()) for k in range(cc - 3, cc + 4) if 1 <= k <= NC} | {0})
    needles = np.zeros(len(counts), COLOR_DTYPE)
    needles["colors"] = rng.integers(0, 65536, (len(counts), NC, 4))
    needles["numColors"] = counts
    live = np.nonzero(ids)[0]
    removable = ids[live[5::11]] if n > 2 else ids[:0]
    return descs, ids, needles, removable


def removed(descs, ids, victims):
    """the index after remove(victims): id 0 and the descriptor cleared, in place"""
    d, i = descs.copy(), ids.copy()
    hit = np.isin(i, np.asarray(victims, np.uint32)) & (i != 0)
    d[hit] = np.zeros((), COLOR_DTYPE)
    i[hit] = 0
    return d, i


# ---- the cut of find_batch ----------------------------------------------------------------------------------------------
def reference_cut(scores, ids, k):
    """(out_ids [nq, k], out_scores [nq, k], counts [nq]) from float scores: every entry with a finite score and id != 0
    is a match; the first min(count, k) in (score, id) order, the rest 0"""
    s = int_scores(scores)
    ids = np.asarray(ids, np.uint32)
    nq = s.shape[0]
    oi = np.zeros((nq, k), np.uint32)
    os_ = np.zeros((nq, k), np.int32)
    counts = np.zeros(nq, np.uint32)
    for q in range(nq):
        v = np.nonzero((s[q] >= 0) & (ids != 0))[0]
        counts[q] = len(v)
        order = v[np.lexsort((ids[v], s[q, v]))][:k]
        oi[q, : len(order)] = ids[order]
        os_[q, : len(order)] = s[q, order]
    return oi, os_, counts


def route(scores, ids, k):
    """per needle: "none" (no match, or k = 0: nothing to cut), "window" (answered from the candidate list) or "full"
    (color_full_sort_one).  The rule of cbh_color_find_batch: T = the k-th smallest score when there are k matches and it
    lies in the WIN bins from the needle's minimum, otherwise everything; the candidate list iff 1 <= k <= CAND_CAP and
    the matches at or under T number at most CAND_CAP"""
    s = int_scores(scores)
    ids = np.asarray(ids, np.uint32)
    out = []
    for q in range(s.shape[0]):
        v = np.sort(s[q][(s[q] >= 0) & (ids != 0)])
        if k == 0 or len(v) == 0:
            out.append("none")
            continue
        if len(v) >= k and v[k - 1] - v[0] < WIN:
            ncand = int((v <= v[k - 1]).sum())
        else:
            ncand = len(v)
        out.append("window" if 1 <= k <= CAND_CAP and ncand <= CAND_CAP else "full")
    return out


def predicted_counters(scores, ids, k):
    """(full sorts, window cuts) the call adds to "color_full_sorts" / "color_window_cuts\""""
    r = route(scores, ids, k)
    return r.count("full"), r.count("window")


# The steerable family: a needle of M equal colours (L = 0) against entries of M - 2 equal colours that differ from it in
# L only.  The needle side sums: score = 1 + M d (in float32, d = L * 100 / 65535), 0.049 per step of L, so every integer
# score from 1 to 3201 has some twenty L values.  _L_OF[s] is one of them, found with np_scores itself.
M = 32
U0, V0 = 30000, 30000


def family_needle(num=M, l=0):
    d = np.zeros((), COLOR_DTYPE)
    d["colors"][:num] = (l, U0, V0, 1)
    d["numColors"] = num
    return d


def family_entries(ls, num=M - 2):
    ls = np.asarray(ls)
    d = np.zeros(len(ls), COLOR_DTYPE)
    d["colors"][:, :num, 0] = ls[:, None]
    d["colors"][:, :num, 1] = U0
    d["colors"][:, :num, 2] = V0
    d["colors"][:, :num, 3] = 1
    d["numColors"] = num
    return d


def _l_of():
    if "l_of" not in _cache:
        grid = np.arange(0, 65536, 8)
        s = int_scores(np_scores(family_needle().reshape(1), family_entries(grid)))[0]
        assert (np.diff(s) >= 0).all() and s[0] == 1 and s[-1] >= 3200
        tab = np.full(int(s[-1]) + 1, -1, np.int64)
        tab[s] = grid                       # (the last grid point of every score)
        assert (tab[1:] >= 0).all()
        _cache["l_of"] = tab
    return _cache["l_of"]


def entries_scoring(targets, num=M - 2):
    """entries whose int score against family_needle() is targets[i]"""
    return family_entries(_l_of()[np.asarray(targets, np.int64)], num)


SELECT_NAMES = ("typical", "kth_last_bin", "kth_outside_window", "kth_outside_many", "fewer_valid_than_k", "ties_4096",
                "ties_4097", "k0", "k1", "k4096", "k4097", "k_gt_n", "min_has_id0", "zero_needle_between", "nq65", "chunks8")
Case = namedtuple("Case", "name descs ids needles k expect_path remove")
# expect_path: the route of needle 0 ("window" | "full" | "none"); remove: ids to remove() after loading


def _ids(n, first=1):
    return np.arange(first, first + n, dtype=np.uint32)


def _shuffled(rng, descs, ids):
    p = rng.permutation(len(ids))
    return descs[p], ids[p]


def select_cases():
    """named cases of cbh_color_find_batch, n <= 9000 each"""
    if "select" in _cache:
        return _cache["select"]
    rng = np.random.default_rng(7)
    nd1 = family_needle().reshape(1)
    cases = []

    def add(name, targets, k, expect, needles=nd1, ids=None, remove=(), nums=None):
        targets = np.asarray(targets, np.int64)
        d = entries_scoring(targets)
        if nums is not None:
            d["numColors"] = nums
        i = _ids(len(d)) if ids is None else np.asarray(ids, np.uint32)
        d, i = _shuffled(rng, d, i)
        cases.append(Case(name, d, i, np.asarray(needles, COLOR_DTYPE).reshape(-1), k, expect,
                          np.asarray(remove, np.uint32)))

    # a typical call: 3000 entries spread over 600 scores, k = 8
    add("typical", rng.integers(40, 640, 3000), 8, "window")
    # the k-th score in the window's last bin, and one past it (threshold INT_MAX: everything is a candidate)
    spread = np.r_[100, rng.integers(101, 2147, 6)]
    add("kth_last_bin", np.r_[spread, 100 + WIN - 1, rng.integers(100 + WIN, 3000, 500)], 8, "window")
    add("kth_outside_window", np.r_[spread, 100 + WIN, rng.integers(100 + WIN + 1, 3000, 500)], 8, "window")
    # ... with more matches than the candidate list holds: the full sort
    add("kth_outside_many", np.r_[spread, 100 + WIN, rng.integers(100 + WIN + 1, 3200, 4500)], 8, "full")
    # fewer matches than k: entries the needle cannot match (colour counts differ by 3) around five that it can
    nums = np.full(300, M - 3)
    nums[:5] = M - 2
    add("fewer_valid_than_k", rng.integers(10, 900, 300), 8, "window", nums=nums)
    # ties at the k-th score: exactly CAND_CAP entries at or under it, and one more
    add("ties_4096", np.r_[[50] * 3, [77] * (CAND_CAP - 3), rng.integers(78, 900, 300)], 5, "window")
    add("ties_4097", np.r_[[50] * 3, [77] * (CAND_CAP - 2), rng.integers(78, 900, 300)], 5, "full")
    # k at its edges over 5000 entries; the 4096th and 4097th scores differ, so k = 4096 fills the candidate list exactly
    edge = np.r_[np.sort(rng.integers(20, 1500, CAND_CAP)), rng.integers(1501, 3000, 5000 - CAND_CAP)]
    for k, expect in ((0, "none"), (1, "window"), (CAND_CAP, "window"), (CAND_CAP + 1, "full")):
        add(f"k{k}", edge, k, expect)
    add("k_gt_n", rng.integers(10, 900, 10), 50, "window")
    # the lowest score belongs to an entry whose id is 0, the next lowest to one that is removed; counted into the
    # minimum, either would push the k-th score (true minimum + WIN - 1) out of the window and, with more than CAND_CAP
    # matches, the needle into the full sort
    t = np.r_[1, 2, 100, rng.integers(101, 2147, 6), 100 + WIN - 1, rng.integers(100 + WIN, 3200, 4500)]
    ids = _ids(len(t))
    ids[0] = 0
    add("min_has_id0", t, 8, "window", ids=ids, remove=[2])
    # a needle without colours between scoring ones; needles of 32, 31 and 30 colours see different scores
    three = np.stack([family_needle(), family_needle(0), family_needle(M - 1)])
    add("zero_needle_between", rng.integers(40, 640, 700), 8, "window", needles=three)
    # 65 needles: colour counts 30..32 and L offsets, a colourless one, and every fifth with 27 colours, which matches
    # nothing here
    many = np.stack([family_needle(M - (q % 3), l=40 * q) for q in range(65)])
    many[13] = family_needle(0)
    many[::5] = family_needle(M - 5)
    add("nq65", rng.integers(40, 2000, 2500), 6, "none", needles=many)
    # 8 needles for the chunk loop: entries of 28 colours, CAND_CAP + 100 of them at one low score, are matched by the
    # 30-colour needles 4 and 7 only (more ties than candidates: full sort); the 32-colour needles see the 30-colour
    # entries alone (window)
    nums = np.r_[np.full(CAND_CAP + 100, M - 4), np.full(600, M - 2)]
    mixed = np.stack([family_needle(M, l=25 * q) for q in range(8)])
    mixed[4] = family_needle(M - 2, l=10)
    mixed[7] = family_needle(M - 2, l=300)
    add("chunks8", np.r_[np.full(CAND_CAP + 100, 3), rng.integers(100, 1200, 600)], 5, "window", needles=mixed,
        nums=nums)
    assert tuple(c.name for c in cases) == SELECT_NAMES
    _cache["select"] = {c.name: c for c in cases}
    return _cache["select"]


def case_index(case):
    """(descs, ids) of a case as the index holds them once case.remove is removed"""
    return removed(case.descs, case.ids, case.remove) if len(case.remove) else (case.descs, case.ids)
