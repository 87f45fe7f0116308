"""The prefilter drain's row walk (`work` in prefilter_body, cbird_amd/csrc/hamm64_mfma.hip) on the GPU: the rows of an
item's chain are first compared on their 32-bit fold, and only the survivors on all 64 bits.  Every prefilter variant runs
the same drain, so every case runs once per variant, forced as the variants' own tests force them ("scan_mfma" 2 with
"scan_mfma_pre_max" 32 | "scan_pre16" 1 | "scan_pre48" 1), and the FULL record multiset is compared against
scan_layout.reference_records and against the same call on the three-field kernel.  The arithmetic on paper:
tests/test_prefilter_walk_model.py.

Shapes: n = 1024 is one workgroup, 1024 + 37 the ragged one; nq = 128 one step, 129 a lone last pair, 640 five steps.
A wave's group k is its rows 64 k .. 64 k + 63; register r of the group, seen from a lane of `half`, is row
32 (r >> 4) + reg_row(r & 15, half) of it; chain 0 = registers 0..16, chain 1 = 17..31; needle j is column j % 32 of field
(j % 128) // 32 of step j // 128, held by lanes column + 32 half."""
import ctypes as C
import functools

import numpy as np
import pytest

import scan_layout as S

ONE = np.uint64(1)
VARIANTS = {
    "pre32": (dict(scan_mfma_pre_max=32), "scan_pre_mask", (1, 2, 7, 8)),
    "pre16": (dict(scan_pre16=1), "scan_pre16_mask", (1, 2, 8)),
    "pre48": (dict(scan_pre48=1), "scan_pre48_mask", (2, 8, 16)),
}
CASES = [(v, t) for v, (_, _, ts) in VARIANTS.items() for t in ts]
SHAPES = tuple((n, nq) for n in (1024, 1024 + 37) for nq in (128, 129, 640))
DEFAULTS = dict(scan_mfma=1, scan_mfma_pre_max=-1, scan_pre16=-1, scan_pre48=-1)


# ---- the library on one kernel ------------------------------------------------------------------------------------------
def _set(L, **knobs):
    from cbird_amd import _lib

    for k, v in knobs.items():
        assert L.cbh_set_tuning(k.encode(), v) == _lib.CBH_OK, k


def _get(L, key):
    v = C.c_longlong(0)
    assert L.cbh_get_tuning(key.encode(), C.byref(v)) == 0
    return v.value


@pytest.fixture
def lib(gpu):
    from cbird_amd import _lib

    L = _lib.lib()
    try:
        yield L
    finally:
        _set(L, **DEFAULTS)


def _force(L, variant):
    _set(L, **DEFAULTS)
    _set(L, scan_mfma=2, **VARIANTS[variant][0])


def _took(L, variant, thresh):
    return bool((_get(L, VARIANTS[variant][1]) >> thresh) & 1) and (
        variant != "pre32" or not ((_get(L, "scan_pre16_mask") | _get(L, "scan_pre48_mask")) >> thresh) & 1)


def _scan(L, idx, needles, thresh, cap):
    import torch

    from cbird_amd import _lib

    dq = torch.from_numpy(needles.view(np.int64)).cuda()
    drec = torch.zeros(max(1, cap), dtype=torch.int64, device="cuda")
    dtot = torch.zeros(1, dtype=torch.int64, device="cuda")
    _lib.check(L.cbh_idx64_scan_dev(idx.handle, dq.data_ptr(), len(needles), thresh, drec.data_ptr(), cap,
                                    dtot.data_ptr(), None), "scan")
    tot = int(dtot.item())
    return tot, np.sort(drec[:min(tot, cap)].cpu().numpy().view(np.uint64))


def _same(name, got, want):
    if not np.array_equal(got, want):
        missing, extra = S.multiset_diff(got, want)
        raise AssertionError(f"{name}: {len(got)} records, {len(want)} expected; {len(missing)} missing "
                             f"{S.unpack(missing[:4]).tolist()}, {len(extra)} extra {S.unpack(extra[:4]).tolist()}")


def _check(L, gpu, variant, name, hashes, ids, needles, thresh):
    """the variant's records == the reference's == the three-field kernel's, as multisets; -> the reference as a set"""
    want = S.reference_records(hashes, ids, needles, thresh)
    idx = gpu.DctHashIndex()
    idx.load(hashes, ids)
    cap = len(want) + 4096
    _force(L, variant)
    tot, got = _scan(L, idx, needles, thresh, cap)
    assert _took(L, variant, thresh), f"not the {variant} kernel"
    _same(f"{name} {variant} t{thresh} vs reference", got, want)
    assert tot == len(want)
    _set(L, scan_pre16=0, scan_pre48=0, scan_mfma_pre_max=0)
    tot3, got3 = _scan(L, idx, needles, thresh, cap)
    assert not any((_get(L, m) >> thresh) & 1 for m in ("scan_pre_mask", "scan_pre16_mask", "scan_pre48_mask"))
    _same(f"{name} {variant} t{thresh} vs the three-field kernel", got, got3)
    assert tot3 == tot
    return {tuple(x) for x in S.unpack(want).tolist()}


# ---- planted chains -------------------------------------------------------------------------------------------------------
def _slot(wave, group, half, reg):
    return S.WAVE_ROWS * wave + 64 * group + 32 * (reg >> 4) + S.reg_row(reg & 15, half)


def _chain_regs(ch):
    return list(range(17)) if ch == 0 else list(range(17, 32))


def _bits(*bs):
    x = np.uint64(0)
    for b in bs:
        x |= ONE << np.uint64(int(b))
    return x


def _flip_low(rng, d):
    """d distinct bits of the low word: the fold distance is d as well"""
    return _bits(*rng.choice(32, d, replace=False))


def _collide(rng, pairs):
    """`pairs` pairs {i, i + 32}: fold distance 0, 64-bit distance 2 pairs"""
    return _bits(*[b for i in rng.choice(32, pairs, replace=False) for b in (i, i + 32)])


@functools.lru_cache(maxsize=None)
def planted(n, nq, thresh, seed=0):
    """-> slots, ids, needles, plan; plan = [(what, needle, distance, slot)] of every planted pair.  One (wave, group) and
    one needle column per construction; fillers are random.  Every planted chain holds a row at distance 0 or thresh - 1
    of its needle, so that the chain is flagged by every variant's word and all its rows are walked."""
    rng = np.random.default_rng(1000 * thresh + n + nq + seed)
    slots, needles = S._rand64(rng, n), S._rand64(rng, nq)
    ids = np.arange(1, n + 1, dtype=np.uint32)
    steps = nq // 128
    groups = iter([(w, g) for w in range(4) for g in range(4)])
    cols = iter(range(32))
    plan = []

    def chain(ch, field):
        """a fresh group and needle column -> needle (field `field` of step 0), the slots of chain ch's registers as the
        needle's lane of one half sees them, and the slot of any register of the group for that lane"""
        (w, g), c = next(groups), next(cols)
        half = (c + ch) & 1
        return 32 * field + c, [_slot(w, g, half, r) for r in _chain_regs(ch)], lambda r: _slot(w, g, half, r)

    def put(what, j, slot, x):
        slots[slot] = needles[j] ^ x
        plan.append((what, j, int(np.bitwise_count(x)), slot))

    # fold collisions: one pair {i, i + 32} (distance 2), four pairs (distance 8); the second stage alone decides
    for ch in (0, 1):
        j, rows, _ = chain(ch, 2 * ch)
        put("collision anchor", j, rows[3], np.uint64(0))
        put("collision 2", j, rows[0], _collide(rng, 1))
        put("collision 8", j, rows[7], _collide(rng, 4))
        put("collision 8", j, rows[-1], _collide(rng, 4))
    # survivors of one needle in one chain: 1, 2, all 17, all 15 (0: the lower fields behind a top-field carry, below)
    j, rows, _ = chain(0, 1)
    put("one survivor", j, rows[5], np.uint64(0))
    j, rows, _ = chain(1, 3)
    put("two survivors", j, rows[2], np.uint64(0))
    put("two survivors", j, rows[9], _collide(rng, 9))
    for ch in (0, 1):
        j, rows, _ = chain(ch, 1 + ch)
        for k, s in enumerate(rows):  # duplicates of one hash, near rows and far rows, all with the needle's fold
            put("all survive", j, s, (np.uint64(0), _collide(rng, 4), np.uint64(0), _collide(rng, 1), _collide(rng, 11))[k % 5])
    # chain and quad edges: a match at thresh - 1 on registers 0, 15, 16, 17, 31, a near miss at exactly thresh behind it
    for k, reg in enumerate((0, 15, 16, 17, 31)):
        j, rows, at = chain(int(reg > 16), k % 4)
        put(f"edge register {reg}", j, at(reg), _flip_low(rng, thresh - 1))
        # a miss that the first stage drops (fold distance thresh), or one that only the second can drop (a colliding pair
        # in it: fold distance thresh - 2).  Behind register 31: register 0, the other chain.
        if k % 2 == 0 or thresh < 2:
            x = _flip_low(rng, thresh)
        else:
            x = _collide(rng, 1)
            x |= _bits(*[b for b in range(32) if not (x >> np.uint64(b)) & ONE][:thresh - 2])
        put(f"near miss behind {reg}", j, at((reg + 1) % 32), x)
    # a top-field carry with a lower-field match in the same register, one per step, chains alternating; the carried
    # chain's remaining fields have no survivor at all
    for s in range(max(1, steps)):
        ch = s & 1
        (w, g), c = next(groups), next(cols)
        row = _slot(w, g, s & 1, _chain_regs(ch)[(5 * s + 2) % 15])
        for f in (3, s % 3):
            j = 128 * s + 32 * f + c
            needles[j] = slots[row] ^ _flip_low(rng, thresh - 1)
            plan.append(("carry + lower field", j, thresh - 1, row))
    # null needles and removed slots among them
    needles[[5 + 32, nq - 1 if nq % 64 else 77]] = 0
    ids[next(s for what, _, d, s in plan if what == "all survive" and d == 0)] = 0
    return slots, ids, needles, plan


def test_planted_chains_are_where_they_claim():
    """(CPU) every planted pair has its distance; the collisions and far rows share the needle's fold; rows of one chain
    construction are that lane's rows of one chain"""
    for n, nq in SHAPES:
        for thresh in (1, 2, 7, 8, 16):
            slots, ids, needles, plan = planted(n, nq, thresh)
            for what, j, d, s in plan:
                if needles[j] == 0:
                    continue
                assert int(np.bitwise_count(slots[s] ^ needles[j])) == d, what
                if what.startswith(("collision", "all survive", "two", "one")):
                    assert int(S.fold(slots[s])) == int(S.fold(needles[j]))
            rows = [s for w, _, _, s in plan if not w.startswith("carry")]
            assert len(set(rows)) == len(rows)  # no slot planted twice
            whats = {w for w, *_ in plan}
            assert {"collision 2", "collision 8", "all survive", "carry + lower field", "edge register 16"} <= whats
            edge_d = {d for w, _, d, _ in plan if w.startswith("near miss")}
            assert edge_d == {thresh}
            assert sum(1 for w, *_ in plan if w == "all survive") == 17 + 15


@pytest.mark.gpu
@pytest.mark.parametrize("variant,thresh", CASES)
@pytest.mark.parametrize("n,nq", SHAPES)
def test_planted_chains(gpu, lib, variant, thresh, n, nq):
    slots, ids, needles, plan = planted(n, nq, thresh)
    want = _check(lib, gpu, variant, f"planted n{n} nq{nq}", slots, ids, needles, thresh)
    for what, j, d, s in plan:
        expect = d < thresh and needles[j] != 0 and ids[s] != 0 and j < nq
        assert ((j, d, int(ids[s])) in want) == expect, (what, j, d, s)


# ---- the lists at capacity, edge inputs ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("variant,thresh", CASES)
def test_dense_block(gpu, lib, variant, thresh):
    """tests/test_scan_prefilter16.py's block: every lane of every group a descriptor, eight items each, both lists full
    at threshold 1 of the 16-bit prefilter -- and with sixteen true matches of one needle inside it"""
    from test_scan_prefilter16 import dense_block

    slots, ids, needles = dense_block()
    _check(lib, gpu, variant, "dense block", slots, ids, needles, thresh)
    slots = slots.copy()
    for reg in range(16):
        slots[64 + S.reg_row(reg, 1)] = needles[128 + 96 + 9]
    want = _check(lib, gpu, variant, "dense block with matches", slots, ids, needles, thresh)
    assert sum(1 for j, d, _ in want if j == 128 + 96 + 9 and d == 0) == 16


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["list_at_its_maximum", "carry_hides_a_match", "many_rows_one_needle"])
def test_event_fixtures(gpu, lib, variant, name):
    from test_scan_prefilter_events import EVENT_FIXTURES

    fx = EVENT_FIXTURES[name]()
    want = _check(lib, gpu, variant, name, fx.hashes, fx.ids, fx.needles, fx.thresh)
    if "records" in fx.target:
        assert sorted(want) == fx.target["records"]


@pytest.mark.gpu
@pytest.mark.parametrize("variant,thresh", CASES)
@pytest.mark.parametrize("name", ["padding_385", "padding_769", "removed_null_masked"])
def test_null_and_padding_needles(gpu, lib, variant, thresh, name):
    """n and nq off every tile, a lone last pair, needles of hash 0 and low popcount, removed slots"""
    fx = S.BUILDERS[name]()
    _check(lib, gpu, variant, name, fx.hashes, fx.ids, fx.needles, thresh)


@pytest.mark.gpu
@pytest.mark.parametrize("variant,thresh", CASES)
def test_needle_masks(gpu, lib, variant, thresh):
    """find_batch(masks=...): mask_ok behind the second stage"""
    fx = S.BUILDERS["removed_null_masked"]()
    want = S.unpack(S.reference_records(fx.hashes, fx.ids, fx.needles, thresh, fx.masks))
    counts = np.bincount(want[:, 0], minlength=len(fx.needles))
    idx = gpu.DctHashIndex()
    idx.load(fx.hashes, fx.ids)
    _force(lib, variant)
    gi, gs, gc = idx.find_batch(fx.needles, thresh, max(1, int(counts.max())), masks=fx.masks)
    assert _took(lib, variant, thresh)
    assert gc.tolist() == counts.tolist()
    w = want[np.lexsort((want[:, 2], want[:, 1], want[:, 0]))]
    starts = np.r_[0, np.cumsum(counts)]
    for j in np.nonzero(counts)[0].tolist():
        a, b = starts[j], starts[j + 1]
        assert gi[j, :b - a].tolist() == w[a:b, 2].tolist() and gs[j, :b - a].tolist() == w[a:b, 1].tolist(), j


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_keep_id0(gpu, orc, lib, variant):
    """DctFeaturesIndex scans with keep_id0: removed slots still vote"""
    from cbird_amd import synth

    m, k = 40, 120
    h, _ = synth.make_hashes(m * k, seed=15, planted_frac=0.4, max_dist=7)
    ids = np.repeat(np.arange(1, m + 1, dtype=np.uint32), k)
    media = [gpu.Media(id=i, keyPointHashes=h[ids == i].tolist()) for i in range(1, m + 1)]
    idx = gpu.DctFeaturesIndex()
    idx.load([])
    idx.add(media)
    idx.remove([3, 9])
    ids_after = ids.copy()
    ids_after[np.isin(ids, [3, 9])] = 0
    _force(lib, variant)
    for thresh in VARIANTS[variant][2][1:]:
        p = gpu.SearchParams(dctThresh=thresh)
        for nd in media[:12:3]:
            got = idx.find_batch([nd], p)[0]
            assert _took(lib, variant, thresh)
            wi, ws = orc.fdct_find(h, ids_after, np.array(nd.keyPointHashes, np.uint64), nd.id, thresh)
            assert [x.mediaId for x in got] == wi.tolist() and [x.score for x in got] == ws.tolist(), nd.id
