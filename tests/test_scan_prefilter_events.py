"""The prefilter kernel's candidate events (k_hamm64_mfma<true>, cbird_amd/csrc/hamm64_mfma.hip): every hit lane of a
group appends ONE descriptor {flag bits of its two reduction chains, lane | group | step}, and the drain re-checks ALL
rows of a flagged chain (registers 0..16 / 17..31 of the group) against the needles of the flagged fields.  What that
rule can get wrong is a row it does not walk, a row it walks twice, a field it drops behind a carry and a list that
overflows -- so the inputs here put candidates in every lane of every group of every step, hide a match behind the top
field's carry, and give one needle several rows of one lane's chain.  The GPU tests compare the FULL record multiset
with scan_layout.reference_records: no sampling, no tolerance.

(scan_layout.prefilter_model describes the pending list of the kernel BEFORE this rule -- one descriptor per flagged
register -- and stays as the record of it; the model of the rule now is pending_trace() below.)"""
import ctypes as C

import numpy as np
import pytest

import scan_layout as S

PEND_MAX = 319  # 63 a drain leaves + 4 groups x 64 lanes (kPendCap = 320 in the kernel)
CHAIN_REGS = (range(0, 17), range(17, 32))  # the two OR chains of a group's 32 accumulator registers


# ---- the rule, in numpy -------------------------------------------------------------------------------------------------
def hit_lanes(hashes, needles, thresh):
    """{(wave, chunk, step, group): hit lanes} of one prefilter launch: the lanes whose 32 registers x 4 fields hold a
    fold candidate (padding slots and needles are hash 0; a lone last pair is its own partner)"""
    n, nq = len(hashes), len(needles)
    n_pairs = S._cdiv(nq, 64)
    ppc = S.prefilter_pairs_per_chunk(n, nq)
    sf = np.zeros(S._cdiv(n, S.WAVE_ROWS) * S.WAVE_ROWS, np.uint32)
    sf[:n] = S.fold(hashes)
    nf = np.zeros(n_pairs * 64, np.uint32)
    nf[:nq] = S.fold(needles)
    i, j = S.pairs_below(sf, nf, thresh)
    P = j // 64
    chunk, rel = P // ppc, P % ppc
    W, rw = i // S.WAVE_ROWS, i % S.WAVE_ROWS
    _, half = S.row_reg(rw % 32)
    lane = (j % 32) + 32 * half
    key = np.unique(np.stack([W, chunk, rel // 2, rw // 64, lane], axis=1), axis=0)
    out = {}
    for w, c, s, g, _ in key.tolist():
        out[(w, c, s, g)] = out.get((w, c, s, g), 0) + 1
    return out


def pending_trace(hashes, needles, thresh):
    """(the most descriptors any wave has pending, the most one step adds): a group adds one per hit lane, the list is
    drained at the end of a step once >= 64 are pending (it keeps npend & 63) and emptied at the end of a needle chunk"""
    ev = hit_lanes(hashes, needles, thresh)
    peak = step_max = 0
    inst, npend, cur, added = None, 0, None, 0
    for (w, c, s, g) in sorted(ev):
        if (w, c) != inst:
            inst, cur, npend, added = (w, c), s, 0, 0
        elif s != cur:
            cur, added = s, 0
            if npend >= 64:
                npend &= 63
        npend += ev[(w, c, s, g)]
        added += ev[(w, c, s, g)]
        peak, step_max = max(peak, npend), max(step_max, added)
    return peak, step_max


# ---- inputs -------------------------------------------------------------------------------------------------------------
def every_lane_hits(thresh, seed=21):
    """uniform random hashes at a threshold where a lane's 128 pairs of a group nearly always hold a fold candidate
    (fold-candidate rate 0.055 at 12, 0.43 at 16), the ragged sizes of scan_layout.padding_guards, a few dozen planted
    near-copies: padding rows, padding needles and the lone last pair are all among the candidates"""
    rng = np.random.default_rng(seed)
    n, nq = 2 * 1024 + 256 + 37, 385
    slots, needles = S._rand64(rng, n), S._rand64(rng, nq)
    src = rng.choice(n, 48, replace=False)
    dst = rng.choice(nq, 48, replace=False)
    for s, d in zip(src.tolist(), dst.tolist()):
        needles[d] = S._near(rng, slots[s], 1, thresh - 1)[0]
    needles[nq - 1] = S._near(rng, slots[n - 1], 1, 2)[0]  # the single last pair of the launch
    ids = np.arange(1, n + 1, dtype=np.uint32)
    return S.Fixture(f"every_lane_t{thresh}", slots, ids, needles, thresh, prefilter=True)


def list_at_its_maximum(seed=22):
    """Threshold 4, one wave: step 0 leaves 63 descriptors (63 hit lanes in group 0: A on the rows the half-0 lanes see,
    B on those of the half-1 lanes, needles A in all 32 columns of field 0 and B in 31 columns of field 1), then every
    lane of every group of step 1 is a hit lane (C on one row of either lane half in each group's second tile, needles C
    in all columns of field 2): 63 + 4 x 64 = 319 pending."""
    thresh = 4
    rng = np.random.default_rng(seed)
    A, B, Cc = S._rand64(rng, 3)
    slots, needles = S._rand64(rng, S.WAVE_ROWS), S._rand64(rng, 256)
    fixed_s, fixed_n = np.zeros(S.WAVE_ROWS, bool), np.zeros(256, bool)
    r = np.arange(32)
    slots[r[(r >> 2) & 1 == 0]] = A  # tile 0 of group 0
    slots[r[(r >> 2) & 1 == 1]] = B
    fixed_s[:32] = True
    for g in range(4):
        for rit in (1, 5):  # reg_row(1, 0), reg_row(1, 1)
            slots[64 * g + 32 + rit] = Cc
            fixed_s[64 * g + 32 + rit] = True
    needles[0:32], needles[32:63], needles[128 + 64:128 + 96] = A, B, Cc
    fixed_n[0:63] = True
    fixed_n[128 + 64:128 + 96] = True
    S._clean_fillers(rng, slots, needles, ~fixed_s, ~fixed_n, thresh)
    return S.Fixture("list_at_its_maximum", slots, np.arange(1, S.WAVE_ROWS + 1, dtype=np.uint32), needles, thresh,
                     prefilter=True)


def carry_hides_a_match(seed=23):
    """Threshold 5.  In every step s and at a different (wave, group, row, column c) each time: a slot EQUAL to needle c of
    tile 0 of the step whose fold is also within the threshold of needle c of tile 3 -- same lane, same register; the top
    field carries into the exponent and the register's lower flag bits are unreadable.  Tile 3's needle shares the
    slot's fold exactly but is 2 popc(r) >= 10 bits away on 64 bits: only the hidden match is a record."""
    thresh = 5
    rng = np.random.default_rng(seed)
    steps, n = 6, 2 * S.WAVE_ROWS
    slots, needles = S._rand64(rng, n), S._rand64(rng, 128 * steps)
    fixed_s, fixed_n = np.zeros(n, bool), np.zeros(128 * steps, bool)
    want = []
    for s in range(steps):
        row = int(rng.integers(0, n))
        while fixed_s[row]:
            row = int(rng.integers(0, n))
        c = int(rng.integers(0, 32))
        H = slots[row]
        rr = np.uint64(int(rng.integers(1, 1 << 32)) | 0x1F)  # popc >= 5
        needles[128 * s + c] = H
        needles[128 * s + 96 + c] = H ^ (rr | (rr << np.uint64(32)))
        fixed_s[row] = True
        fixed_n[[128 * s + c, 128 * s + 96 + c]] = True
        want.append((128 * s + c, 0, row + 1))
    S._clean_fillers(rng, slots, needles, ~fixed_s, ~fixed_n, thresh)
    fx = S.Fixture("carry_hides_a_match", slots, np.arange(1, n + 1, dtype=np.uint32), needles, thresh, prefilter=True)
    fx.target["records"] = sorted(want)
    return fx


def many_rows_one_needle(seed=24):
    """Threshold 4.  Needle X (step 1, field 1, column 7) equals the slots at rows 0, 1, 2, 3, 8, 16 of a group's first
    tile and rows 0, 1, 24 of its second: all rows of lane 7 (half 0) -- registers 0..3, 4, 8 and 16 (which closes the first
    chain), 17 and 28 (second chain).  Needle Y (field 2, column 30) the same shifted by 4 rows: lane 62 (half 1)."""
    thresh = 4
    rng = np.random.default_rng(seed)
    X, Y = S._rand64(rng, 2)
    n = 2 * S.WAVE_ROWS
    slots, needles = S._rand64(rng, n), S._rand64(rng, 384)
    fixed_s, fixed_n = np.zeros(n, bool), np.zeros(384, bool)
    g0 = S.WAVE_ROWS + 64 * 2  # wave 1, group 2
    rows = [0, 1, 2, 3, 8, 16, 32 + 0, 32 + 1, 32 + 24]
    for k in rows:
        slots[g0 + k], slots[g0 + k + 4] = X, Y
        fixed_s[[g0 + k, g0 + k + 4]] = True
    qx, qy = 128 + 32 + 7, 128 + 64 + 30
    needles[qx], needles[qy] = X, Y
    fixed_n[[qx, qy]] = True
    S._clean_fillers(rng, slots, needles, ~fixed_s, ~fixed_n, thresh)
    fx = S.Fixture("many_rows_one_needle", slots, np.arange(1, n + 1, dtype=np.uint32), needles, thresh, prefilter=True)
    fx.target["records"] = sorted([(qx, 0, g0 + k + 1) for k in rows] + [(qy, 0, g0 + k + 5) for k in rows])
    return fx


EVENT_FIXTURES = {
    "every_lane_t12": lambda: every_lane_hits(12),
    "every_lane_t16": lambda: every_lane_hits(16),
    "list_at_its_maximum": list_at_its_maximum,
    "carry_hides_a_match": carry_hides_a_match,
    "many_rows_one_needle": many_rows_one_needle,
}
PRE_BUILDERS = ["peak_r32", "peak_r33", "peak_r47", "peak_r63", "peak_repl", "chunk_at_group0", "chunk_at_group1",
                "chunk_at_group2", "chunk_at_group3", "dense_all_fields", "dense_field3_only", "second_tile_only",
                "padding_385", "padding_769", "removed_null_masked"]


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_prefilter_builders_are_the_ones_listed():
    assert PRE_BUILDERS == [k for k in S.BUILDERS if S.BUILDERS[k]().prefilter]


def test_chain_rows_are_runs_of_four():
    """the drain walks a chain by register quads: register r of a group sits at wave row base + 8 (r >> 2) + (r & 3),
    base = 64 group + 4 half -- the C/D layout restated; the two chains cover a lane's 32 rows once"""
    for half in (0, 1):
        seen = []
        for chain in CHAIN_REGS:
            for r in chain:
                t, g = r >> 4, r & 15
                assert 4 * half + 8 * (r >> 2) + (r & 3) == 32 * t + S.reg_row(g, half)
                seen.append(r)
        assert sorted(seen) == list(range(32))
    assert len(CHAIN_REGS[0]) == 17 and len(CHAIN_REGS[1]) == 15


@pytest.mark.parametrize("name", list(EVENT_FIXTURES))
def test_event_fixtures_reach_what_they_claim(name):
    fx = EVENT_FIXTURES[name]()
    peak, step_max = pending_trace(fx.hashes, fx.needles, fx.thresh)
    assert peak <= PEND_MAX
    ref = S.unpack(S.reference_records(fx.hashes, fx.ids, fx.needles, fx.thresh))
    if name.startswith("every_lane"):
        # every lane of every group of a step: the GPU test exercises 256 appends in one step, on top of a remainder
        assert step_max == 256 and peak >= 256
        ev = hit_lanes(fx.hashes, fx.needles, fx.thresh)
        # waves without padding rows, steps of four whole tiles: a lane's 128 pairs hold a candidate with probability
        # 1 - (1 - 0.055)^128 = 0.9993 at threshold 12, so all 64 lanes hit in 0.956 of those groups (all at 16)
        regular = [v for (w, c, s, g), v in ev.items() if w < len(fx.hashes) // S.WAVE_ROWS and s < len(fx.needles) // 128]
        assert len(regular) == (len(fx.hashes) // S.WAVE_ROWS) * 4 * (len(fx.needles) // 128)
        assert sum(v == 64 for v in regular) >= 0.9 * len(regular)
        m = S.prefilter_model(fx.hashes, fx.needles, fx.thresh)
        assert m.pad_slot > 0 and m.pad_needle > 0
        assert (ref[:, 0] == len(fx.needles) - 1).any() and len(ref) >= 48
    elif name == "list_at_its_maximum":
        assert peak == PEND_MAX and step_max == 256
        assert len(ref) == 32 * 16 + 31 * 16 + 32 * 8
    else:
        assert [tuple(x) for x in ref.tolist()] == fx.target["records"]
    if name == "carry_hides_a_match":
        m = S.prefilter_model(fx.hashes, fx.needles, fx.thresh)
        assert len(m.events) == 6 and all(e.fields == 4 and len(e.lanes) == 1 for e in m.events)  # top field flagged
    if name == "many_rows_one_needle":
        ev = hit_lanes(fx.hashes, fx.needles, fx.thresh)
        assert ev == {(1, 0, 1, 2): 2}  # two hit lanes, one group: nine rows each


def test_pending_bound_holds_for_the_layout_fixtures_at_every_threshold():
    for name in PRE_BUILDERS:
        fx = S.BUILDERS[name]()
        for t in (fx.thresh, 5, 6, 7, 8):
            assert pending_trace(fx.hashes, fx.needles, t)[0] <= PEND_MAX, (name, t)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def forced_prefilter(gpu):
    from cbird_amd import _lib

    L = _lib.lib()
    assert L.cbh_set_tuning(b"scan_mfma", 2) == _lib.CBH_OK
    assert L.cbh_set_tuning(b"scan_mfma_pre_max", 32) == _lib.CBH_OK
    try:
        yield L
    finally:
        L.cbh_set_tuning(b"scan_mfma", 1)
        L.cbh_set_tuning(b"scan_mfma_pre_max", -1)


def _load(gpu, fx):
    idx = gpu.DctHashIndex()
    idx.load(fx.hashes, fx.ids)
    h, i = idx.download()
    assert np.array_equal(h, fx.hashes) and np.array_equal(i, fx.ids)
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
    v = C.c_longlong(0)
    assert L.cbh_get_tuning(b"scan_pre_mask", C.byref(v)) == 0 and (v.value >> thresh) & 1, "not the prefilter kernel"
    return tot, np.sort(drec[:min(tot, cap)].cpu().numpy().view(np.uint64))


def _check(L, gpu, fx, thresh):
    want = S.reference_records(fx.hashes, fx.ids, fx.needles, thresh)
    tot, got = _scan(L, _load(gpu, fx), fx.needles, thresh, len(want) + 4096)
    if not np.array_equal(got, want):
        missing, extra = S.multiset_diff(got, want)
        raise AssertionError(f"{fx.name} t{thresh}: {len(got)} records, {len(want)} expected; {len(missing)} missing "
                             f"{S.unpack(missing[:4]).tolist()}, {len(extra)} extra {S.unpack(extra[:4]).tolist()}")
    assert tot == len(want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EVENT_FIXTURES))
def test_event_fixtures_equal_the_reference(gpu, forced_prefilter, name):
    fx = EVENT_FIXTURES[name]()
    _check(forced_prefilter, gpu, fx, fx.thresh)


@pytest.mark.gpu
@pytest.mark.parametrize("thresh", [5, 6, 7, 8])
@pytest.mark.parametrize("name", PRE_BUILDERS)
def test_layout_fixtures_at_thresholds_5_to_8(gpu, forced_prefilter, name, thresh):
    """the layout fixtures built for the prefilter kernel (dense groups, removed slots, null needles, padding) at the
    thresholds whose route the candidate's cost decides"""
    _check(forced_prefilter, gpu, S.BUILDERS[name](), thresh)


@pytest.mark.gpu
@pytest.mark.parametrize("thresh", [5, 6, 7, 8])
def test_masked_find_batch_on_the_prefilter(gpu, forced_prefilter, thresh):
    """find_batch(masks=...) -> mask_ok in the drain: every match of every needle in (score, mediaId) order"""
    fx = S.BUILDERS["removed_null_masked"]()
    want = S.unpack(S.reference_records(fx.hashes, fx.ids, fx.needles, thresh, fx.masks))
    assert 0 < len(want) < len(S.reference_records(fx.hashes, fx.ids, fx.needles, thresh))
    counts = np.bincount(want[:, 0], minlength=len(fx.needles))
    idx = _load(gpu, fx)
    gi, gs, gc = idx.find_batch(fx.needles, thresh, int(counts.max()), masks=fx.masks)
    assert gc.tolist() == counts.tolist()
    w = want[np.lexsort((want[:, 2], want[:, 1], want[:, 0]))]
    starts = np.r_[0, np.cumsum(counts)]
    for j in np.nonzero(counts)[0].tolist():
        a, b = starts[j], starts[j + 1]
        assert gi[j, :b - a].tolist() == w[a:b, 2].tolist() and gs[j, :b - a].tolist() == w[a:b, 1].tolist(), j
        assert (gi[j, b - a:] == 0).all()
