"""The 16-bit prefilter kernel (k_hamm64_mfma16, PRE16, cbird_amd/csrc/hamm64_mfma.hip) on the GPU, forced with
"scan_mfma" 2, "scan_pre16" 1: the FULL record multiset of every case against scan_layout.reference_records AND against the
same call with "scan_pre16" 0; "scan_pre16_mask" and "scan_pre_mask" both say the kernel ran.  tests/scan16_layout.py
restates the layout; the arithmetic on paper is in tests/test_scan16_model.py.

Shapes: n = 1024 is one workgroup (4 waves x 8 tiles x 32 rows), 1024 + 37 and 3 x 1024 the ragged and the several;
nq = 128 is one needle quadruple = one step, 129 / 255 / 640 a lone pair behind one, a quadruple one needle short, five.
Thresholds 1, 2, 4, 8: the one the kernel is routed to, its neighbour, the middle, the largest its bias allows.  At 4 and 8
the random fillers are candidates too (P[Bin(16, 1/2) < t] = 1 % and 40 %): every step of every wave drains."""
import ctypes as C
import functools

import numpy as np
import pytest

import scan16_layout as M
import scan_layout as S

THRESHOLDS = (1, 2, 4, 8)
SHAPES = tuple((n, nq) for n in (1024, 1024 + 37, 3 * 1024) for nq in (128, 129, 255, 640))
ONE = np.uint64(1)


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
def lib16(gpu):
    """the matrix-core scan for any size, the 16-bit prefilter for every threshold it can represent"""
    from cbird_amd import _lib

    L = _lib.lib()
    _set(L, scan_mfma=2, scan_pre16=1)
    try:
        yield L
    finally:
        _set(L, scan_mfma=1, scan_pre16=-1, scan_mfma_pre_max=-1)


def _load(gpu, hashes, ids):
    idx = gpu.DctHashIndex()
    idx.load(hashes, ids)
    return idx


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


def _took16(L, thresh):
    return bool((_get(L, "scan_pre16_mask") >> thresh) & 1)


def _scan16(L, idx, needles, thresh, cap):
    out = _scan(L, idx, needles, thresh, cap)
    assert _took16(L, thresh), "not the 16-bit prefilter kernel"
    assert (_get(L, "scan_pre_mask") >> thresh) & 1, "a 16-bit prefilter launch counts as a prefilter launch"
    assert not (_get(L, "scan_pre48_mask") >> thresh) & 1
    return out


def _scan_without(L, idx, needles, thresh, cap):
    _set(L, scan_pre16=0)
    try:
        out = _scan(L, idx, needles, thresh, cap)
        assert not _took16(L, thresh)
    finally:
        _set(L, scan_pre16=1)
    return out


def _same(name, got, want):
    if not np.array_equal(got, want):
        missing, extra = S.multiset_diff(got, want)
        raise AssertionError(f"{name}: {len(got)} records, {len(want)} expected; {len(missing)} missing "
                             f"{S.unpack(missing[:4]).tolist()}, {len(extra)} extra {S.unpack(extra[:4]).tolist()}")


def _check(L, gpu, name, hashes, ids, needles, thresh):
    want = S.reference_records(hashes, ids, needles, thresh)
    idx = _load(gpu, hashes, ids)
    cap = len(want) + 4096
    tot, got = _scan16(L, idx, needles, thresh, cap)
    _same(f"{name} t{thresh} vs reference", got, want)
    assert tot == len(want)
    tot0, got0 = _scan_without(L, idx, needles, thresh, cap)
    _same(f"{name} t{thresh} vs scan_pre16 0", got, got0)
    assert tot0 == tot
    return {tuple(x) for x in S.unpack(want).tolist()}


def _flip(rng, h, d):
    """h with d distinct random bits flipped (64-bit distance d)"""
    h = np.uint64(h)
    for b in rng.choice(64, d, replace=False):
        h ^= ONE << np.uint64(int(b))
    return h


def _row_in_chain(rng, n, chain):
    while True:
        row = int(rng.integers(0, n))
        if M.row_chain(row % S.WAVE_ROWS) == chain:
            return row


# ---- (a) planted pairs ------------------------------------------------------------------------------------------------------
def planted(n, nq, thresh, seed):
    """needles at 64-bit distance t - 1 / t / t + 1 from a slot, in every field P Q R S (needle tile of its quadruple) and
    on rows of both reduction chains (registers 0..16 | 17..31); unrelated hashes around them"""
    rng = np.random.default_rng(seed)
    slots, needles = S._rand64(rng, n), S._rand64(rng, nq)
    free = list(rng.permutation(nq).tolist())
    plan = []
    for field in range(4):
        for chain in range(2):
            for d in (thresh - 1, thresh, thresh + 1):
                j = next(x for x in free if (x // 32) % 4 == field)
                free.remove(j)
                row = _row_in_chain(rng, n, chain)
                needles[j] = _flip(rng, slots[row], d)
                plan.append((j, d, row))
    return slots, np.arange(1, n + 1, dtype=np.uint32), needles, plan


@pytest.mark.gpu
@pytest.mark.parametrize("thresh", THRESHOLDS)
@pytest.mark.parametrize("n,nq", SHAPES)
def test_a_planted_pairs(gpu, lib16, n, nq, thresh):
    slots, ids, needles, plan = planted(n, nq, thresh, 1000 * thresh + nq + n)
    want = _check(lib16, gpu, f"planted n{n} nq{nq}", slots, ids, needles, thresh)
    for j, d, row in plan:
        assert ((j, d, row + 1) in want) == (d < thresh)
    assert {(j // 32) % 4 for j, _, _ in plan} == {0, 1, 2, 3}
    assert {M.row_chain(row % S.WAVE_ROWS) for _, _, row in plan} == {0, 1}


# ---- (b) one register: a top-field hit above a lower-field hit, complements, fold16 collisions ---------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("thresh", THRESHOLDS)
def test_b_top_field_and_lower_field_in_one_register(gpu, lib16, thresh):
    """same row, same column: a match in the top field S (the carry into the exponent, after which the register's lower
    fields are unreadable) and one in field 0 / 1 / 2; in a fourth quadruple the complement word (d16 = 16, the smallest a
    field gets: 16 + b, no borrow) sits in the fields around a match"""
    rng = np.random.default_rng(17 + thresh)
    n, nq = 1024 + 37, 640
    slots, needles = S._rand64(rng, n), S._rand64(rng, nq)
    must = []
    for quad in range(4):
        for chain in range(2):
            row = _row_in_chain(rng, n, chain)
            c = int(rng.integers(0, 16)) + 16 * chain
            H = slots[row]
            if quad < 3:
                needles[128 * quad + 96 + c] = _flip(rng, H, thresh - 1)
                needles[128 * quad + 32 * quad + c] = _flip(rng, H, thresh - 1)
                must += [(128 * quad + 96 + c, thresh - 1, row + 1), (128 * quad + 32 * quad + c, thresh - 1, row + 1)]
            else:
                for f in (0, 1, 3):
                    needles[128 * quad + 32 * f + c] = H ^ np.uint64(0xFFFF)  # every element of fold16 flipped
                    assert int(M.d16(H, needles[128 * quad + 32 * f + c])) == 16
                needles[128 * quad + 64 + c] = _flip(rng, H, thresh - 1)
                must.append((128 * quad + 64 + c, thresh - 1, row + 1))
    ids = np.arange(1, n + 1, dtype=np.uint32)
    assert set(must) <= _check(lib16, gpu, "one register", slots, ids, needles, thresh)


COLLISIONS = (("i_i16", (0, 16), 2), ("i_i32", (0, 32), 2), ("all_four", (0, 16, 32, 48), 4))


@pytest.mark.gpu
@pytest.mark.parametrize("thresh", THRESHOLDS)
def test_b_fold16_collisions(gpu, lib16, thresh):
    """a ^ b = bits {i, i + 16}, {i, i + 32}, {i, i + 16, i + 32, i + 48}: fold16 distance 0, a candidate at every
    threshold, a match only where the 64-bit distance (2, 2, 4) is under it"""
    rng = np.random.default_rng(23 + thresh)
    n, nq = 1024, 255
    slots, needles = S._rand64(rng, n), S._rand64(rng, nq)
    plan = []
    free = list(rng.permutation(nq).tolist())
    for k, (_, offs, d) in enumerate(COLLISIONS):
        for field in range(4):
            i = int(rng.integers(0, 16))
            j = next(x for x in free if (x // 32) % 4 == field)
            free.remove(j)
            row = _row_in_chain(rng, n, (k + field) & 1)
            x = np.uint64(0)
            for o in offs:
                x |= ONE << np.uint64(i + o)
            needles[j] = slots[row] ^ x
            assert int(M.d16(slots[row], needles[j])) == 0
            plan.append((j, d, row))
    want = _check(lib16, gpu, "collisions", slots, np.arange(1, n + 1, dtype=np.uint32), needles, thresh)
    for j, d, row in plan:
        assert ((j, d, row + 1) in want) == (d < thresh)
    assert any(d >= thresh for _, d, _ in plan) == (thresh <= 4)


# ---- (c) the lists at their capacities ------------------------------------------------------------------------------------------
def _wave_row(group, half, chain):
    """a row of wave 0 that lanes of `half` hold in chain `chain` of `group`: register 0 of tile 0 | 17 = 1 of tile 1"""
    return 64 * group + 32 * chain + S.reg_row(chain, half)


def _with_fold16(rng, f16, k):
    """k random hashes whose fold16 is f16"""
    return M.kernel_word(rng, k) ^ np.uint64(f16)


@functools.lru_cache(maxsize=None)
def dense_block(seed=51):
    """n = 1024, nq = 256: two steps of wave 0, built from fold16 words that pairs SHARE while their 64-bit distances stay
    >= 8 (random members of fold16's kernel, ~32 bits apart), so that nothing is a match.
    Step 1 is dense: in every group, for both lane halves, one row of each chain shares its word with all 128 needles of
    the second quadruple -- a descriptor from every lane of every group (256), the top field's carry in both chains,
    eight items each.
    Step 0 sets the lists up as tests/test_scan_prefilter_items.py's list_full does: group 0 adds 32 + 31 descriptors of
    one item, group 1 adds 64 with 9 x 8 + 55 x 1 = 127 items.  Its drain works the newest 64 descriptors, one batch of
    items, and keeps 63 descriptors and 63 items; step 1 then ends with 63 + 256 = kPendCap - 1 descriptors and its
    drain's first pass fills the item list to 63 + 512 = kItemCap."""
    rng = np.random.default_rng(seed)
    n, nq = 1024, 256
    for _ in range(50):
        FX, FA, FB, FC, FE = (int(x) for x in rng.choice(1 << 16, 5, replace=False))
        slots, needles = S._rand64(rng, n), S._rand64(rng, nq)
        for g in range(4):
            for half in range(2):
                for chain in range(2):
                    slots[_wave_row(g, half, chain)] = _with_fold16(rng, FX, 1)[0]
        needles[128:] = _with_fold16(rng, FX, 128)
        slots[_wave_row(0, 0, 0) + 1] = _with_fold16(rng, FA, 1)[0]   # (register 1: the row behind the dense one)
        slots[_wave_row(0, 1, 0) + 1] = _with_fold16(rng, FB, 1)[0]
        slots[_wave_row(1, 0, 0) + 1] = _with_fold16(rng, FC, 1)[0]
        slots[_wave_row(1, 0, 1) + 1] = _with_fold16(rng, FC, 1)[0]
        slots[_wave_row(1, 0, 0) + 2] = _with_fold16(rng, FE, 1)[0]
        slots[_wave_row(1, 1, 0) + 1] = _with_fold16(rng, FE, 1)[0]
        needles[0:32] = _with_fold16(rng, FA, 32)            # field 0, lanes (c, half 0) of group 0
        needles[32:63] = _with_fold16(rng, FB, 31)           # field 1, lanes (c, half 1) of group 0: 63 descriptors
        needles[96:96 + 9] = _with_fold16(rng, FC, 9)        # top field, lanes (c < 9, half 0) of group 1, both chains
        # field 2, lanes (c, half 1) of group 1 and, through a second row, (c, half 0): one more item for 9 <= c, nothing
        # new under the carry of c < 9 -- 64 descriptors
        needles[64:96] = _with_fold16(rng, FE, 32)
        w = slots[:S.WAVE_ROWS]
        shared = M.d16(w[:, None], needles[None, :]) == 0
        want = 16 * 128 + 32 + 31 + 2 * 9 + 2 * 32
        if shared.sum() == want and np.bitwise_count(w[:, None] ^ needles[None, :])[shared].min() >= 8:
            return slots, np.arange(1, n + 1, dtype=np.uint32), needles
    raise AssertionError("no dense block without stray candidates")


def test_c_dense_block_reaches_the_capacities():
    """(CPU) at threshold 1 the dense block is exactly what the kernel's lists are sized for; at the others the bounds hold
    with every filler that has become a candidate"""
    slots, ids, needles = dense_block()
    tr = M.trace(slots, needles, 1)[(0, 0)]
    assert tr["pend_peak"] == 63 + 256 == M.PEND_CAP - 1
    assert tr["item_peak"] == M.ITEM_CAP
    assert tr["kept_desc"] == [63, 63] and tr["kept_items"] == [63, 63]
    assert tr["items"] == 63 + 127 + 256 * 8
    for t in THRESHOLDS:
        assert len(S.reference_records(slots[:S.WAVE_ROWS], ids[:S.WAVE_ROWS], needles, t)) == 0
        assert all(v["pend_peak"] <= M.PEND_CAP - 1 and v["item_peak"] <= M.ITEM_CAP for v in M.trace(slots, needles, t).values())


@pytest.mark.gpu
@pytest.mark.parametrize("thresh", THRESHOLDS)
def test_c_dense_block(gpu, lib16, thresh):
    slots, ids, needles = dense_block()
    _check(lib16, gpu, "dense block", slots, ids, needles, thresh)
    # and with true matches inside it: every row of a chain equal to one needle of the top field
    slots = slots.copy()
    for reg in range(16):
        slots[64 + S.reg_row(reg, 1)] = needles[128 + 96 + 9]
    want = _check(lib16, gpu, "dense block with matches", slots, ids, needles, thresh)
    assert sum(1 for j, d, _ in want if j == 128 + 96 + 9 and d == 0) == 16


def _event_fixtures():
    from test_scan_prefilter_events import EVENT_FIXTURES

    return EVENT_FIXTURES


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["list_at_its_maximum", "carry_hides_a_match", "many_rows_one_needle"])
def test_c_duplicate_groups(gpu, lib16, name):
    """the duplicate groups of tests/test_scan_prefilter_events.py (thresholds 4 and 5): equal hashes are candidates of
    any prefilter"""
    fx = _event_fixtures()[name]()
    _check(lib16, gpu, name, fx.hashes, fx.ids, fx.needles, fx.thresh)


# ---- (d) edge inputs --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("thresh", THRESHOLDS)
@pytest.mark.parametrize("name", ["removed_null_masked", "padding_385", "padding_769"])
def test_d_edge_inputs(gpu, lib16, name, thresh):
    """slots of hash 0 and id 0, null and low-popcount needles, n and nq off every tile"""
    fx = S.BUILDERS[name]()
    _check(lib16, gpu, name, fx.hashes, fx.ids, fx.needles, thresh)


@pytest.mark.gpu
@pytest.mark.parametrize("thresh", THRESHOLDS)
def test_d_null_and_padding_needles_of_a_lone_last_pair(gpu, lib16, thresh):
    """nq = 129: the second quadruple holds one needle and 127 padding needles of hash 0, whose fold16 is 0.  Slot Z has
    fold16 0 and is 32 bits from hash 0: a candidate of every padding needle, of the null needles 5 and 70, of the
    needle that equals it and of needle 128, four bits from it.  Removed slots (id 0) hold matches too."""
    rng = np.random.default_rng(61 + thresh)
    n, nq = 1024 + 37, 129
    slots, needles = S._rand64(rng, n), S._rand64(rng, nq)
    Z = np.uint64(0x00FF00FF00FF00FF)
    assert int(M.fold16(Z)) == 0
    slots[300], slots[1030] = Z, Z
    needles[5], needles[70] = 0, 0
    needles[40] = Z
    needles[128] = Z ^ np.uint64(0x0001000100010001)
    ids = np.arange(1, n + 1, dtype=np.uint32)
    ids[1030] = 0
    ids[7::50] = 0
    needles[99] = slots[57]  # a removed slot's twin
    assert ids[57] == 0
    want = _check(lib16, gpu, "lone last pair", slots, ids, needles, thresh)
    assert (40, 0, 301) in want and ((128, 4, 301) in want) == (thresh > 4)
    assert not any(j in (5, 70, 99) or j >= nq for j, _, _ in want)


@pytest.mark.gpu
@pytest.mark.parametrize("thresh", (2, 8))
def test_d_needle_masks(gpu, lib16, thresh):
    """find_batch(masks=...): a d_qmask call, mask_ok in the drain"""
    fx = S.BUILDERS["removed_null_masked"]()
    want = S.unpack(S.reference_records(fx.hashes, fx.ids, fx.needles, thresh, fx.masks))
    counts = np.bincount(want[:, 0], minlength=len(fx.needles))
    idx = _load(gpu, fx.hashes, fx.ids)
    gi, gs, gc = idx.find_batch(fx.needles, thresh, max(1, int(counts.max())), masks=fx.masks)
    assert _took16(lib16, thresh)
    assert gc.tolist() == counts.tolist()
    w = want[np.lexsort((want[:, 2], want[:, 1], want[:, 0]))]
    starts = np.r_[0, np.cumsum(counts)]
    for j in np.nonzero(counts)[0].tolist():
        a, b = starts[j], starts[j + 1]
        assert gi[j, :b - a].tolist() == w[a:b, 2].tolist() and gs[j, :b - a].tolist() == w[a:b, 1].tolist(), j


@pytest.mark.gpu
def test_d_keep_id0(gpu, orc, lib16):
    """DctFeaturesIndex scans with keep_id0: removed slots still vote (src/dctfeaturesindex.cpp)"""
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
    for thresh in (4, 8):
        p = gpu.SearchParams(dctThresh=thresh)
        for nd in media[:12:3]:
            got = idx.find_batch([nd], p)[0]
            assert _took16(lib16, thresh)
            wi, ws = orc.fdct_find(h, ids_after, np.array(nd.keyPointHashes, np.uint64), nd.id, thresh)
            assert [x.mediaId for x in got] == wi.tolist() and [x.score for x in got] == ws.tolist(), nd.id


@pytest.mark.gpu
@pytest.mark.parametrize("thresh", THRESHOLDS)
def test_d_sharded_handle(gpu, orc, lib16, thresh):
    """three shards with ragged shares: one kernel choice and one needle expansion (the 80-byte scratch) for the call"""
    from cbird_amd import _lib

    n, nq = 3 * 1024 + 37, 255
    slots, ids, needles, plan = planted(n, nq, thresh, 77 + thresh)
    ids[5::97] = 0
    _lib.set_default_sharding((1, 3))
    try:
        idx = _load(gpu, slots, ids)
        gi, gs, gc = idx.find_batch(needles, thresh, 8)
    finally:
        _lib.set_default_sharding(None)
    assert _took16(lib16, thresh)
    wi, ws, wc = orc.find64_batch(slots, ids, needles, thresh, 8)
    assert (gc == wc).all() and (gi == wi).all() and (gs == ws).all()


# ---- (e) beyond its thresholds ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_e_threshold_9_falls_back(gpu, lib16):
    """C0 = 2^23 + (24 + b)(1 + 2^6 + 2^12 + 2^18) reaches 2^24 at b = 8: with "scan_pre16" 1 a call at threshold 9 is
    routed as if the knob were -1 (here: the fixed rule's three-field kernel) and answers as ever"""
    n, nq = 1024 + 37, 255
    slots, ids, needles, plan = planted(n, nq, 9, 909)
    want = S.reference_records(slots, ids, needles, 9)
    idx = _load(gpu, slots, ids)
    tot, got = _scan(lib16, idx, needles, 9, len(want) + 4096)
    assert not _took16(lib16, 9) and not (_get(lib16, "scan_pre_mask") >> 9) & 1
    _same("threshold 9", got, want)
    assert tot == len(want) >= 8
    from cbird_amd import _lib

    for bad in (-2, 2, 3):  # the knob takes -1, 0, 1
        assert lib16.cbh_set_tuning(b"scan_pre16", bad) == _lib.CBH_E_INVAL
    tot, got = _scan(lib16, idx, needles, 8, len(want) + 4096)
    assert _took16(lib16, 8)  # (the refused values left it at 1)


# ---- (f) the route as shipped --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_f_default_routing(gpu):
    """2^31 pairs of unrelated hashes (65 536 slots x 32 768 needles) are probed.  The model -- the routing comment in
    hamm64_scan.hip -- gives the 16-bit prefilter  kBase16 + 1.3e4 x r16  ms per 10^12 pairs: at threshold 1, r16 = 2^-16
    = 1.5e-5, that is kBase16 + 0.2, below 0.9 x 8.55 = 7.7 for any kBase16 under 7.5 (the kernel runs half the 32-bit
    prefilter's MFMAs); at threshold 2, r16 = 17 x 2^-16 = 2.6e-4 adds 3.4 ms and would need kBase16 < 4.3.  Threshold 1
    takes the 16-bit prefilter, threshold 2 stays on the 32-bit one.  The records equal the three-field kernel's."""
    from cbird_amd import _lib

    L = _lib.lib()
    assert _get(L, "scan_mfma") == 1
    rng = np.random.default_rng(99)
    n, nq = 65536, 32768
    slots, needles = S._rand64(rng, n), S._rand64(rng, nq)
    for j in range(0, 64):  # a few true matches, so that the record sets are not empty
        needles[j * 512 + j] = slots[j * 1000 + 3] ^ (ONE << np.uint64(j)) * np.uint64(j & 1)
    ids = np.arange(1, n + 1, dtype=np.uint32)
    idx = _load(gpu, slots, ids)
    for thresh, want16 in ((1, True), (2, False)):
        probes = _get(L, "scan_probes")
        tot, got = _scan(L, idx, needles, thresh, 1 << 16)
        assert _get(L, "scan_probes") == probes + 1
        r16 = _get(L, "scan_probe_rate16_e9") * 1e-9
        print(f"threshold {thresh}: r16 = {r16:.3e}, r_cand = {_get(L, 'scan_probe_rate_e9') * 1e-9:.3e}")
        if thresh == 1:
            assert 1.0e-5 <= r16 <= 2.2e-5, r16
        assert _took16(L, thresh) == want16
        assert (_get(L, "scan_pre_mask") >> thresh) & 1
        _set(L, scan_pre16=0, scan_pre48=0, scan_mfma_pre_max=0)
        try:
            tot3, got3 = _scan(L, idx, needles, thresh, 1 << 16)
            assert not _took16(L, thresh) and not (_get(L, "scan_pre_mask") >> thresh) & 1
        finally:
            _set(L, scan_pre16=-1, scan_pre48=-1, scan_mfma_pre_max=-1)
        assert tot == tot3 >= 32
        _same(f"default route t{thresh}", got, got3)
