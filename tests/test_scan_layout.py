"""The 64-bit scan on layout-aligned worst cases (tests/scan_layout.py): fixtures that put matches at chosen waves, tile
groups, lanes and registers of the matrix-core kernels -- the prefilter's pending list at and past its capacity, dense
groups on every path, padding guards -- and the FULL record multiset of every scan path against a plain reference."""
import ctypes as C

import numpy as np
import pytest

import scan_layout as S

GPU_FIXTURES = [k for k in S.BUILDERS if k != "join_wide_value"]


# ---- CPU: the model and the reference ---------------------------------------------------------------------------------
def test_register_rows_cover_each_tile_once():
    rows = sorted(S.reg_row(g, h) for h in (0, 1) for g in range(16))
    assert rows == list(range(32))
    g, h = S.row_reg(np.arange(32))
    assert [S.reg_row(int(a), int(b)) for a, b in zip(g, h)] == list(range(32))


@pytest.mark.parametrize("remainder,peak", [(32, 640), (33, 641), (47, 655), (63, 671)])
def test_pending_peak_builder_reaches_its_target(remainder, peak):
    fx = S.prefilter_pending_peak(remainder)
    m = S.prefilter_model(fx.hashes, fx.needles, fx.thresh)
    assert m.peak == peak and (m.peak > S.PEND_CAP) == (remainder > 32)
    (ev,) = [e for e in m.events if e.peak == peak]
    assert (ev.step, ev.group, ev.before, len(ev.lanes)) == (1, 3, remainder + 96, 32)
    # the kernel's rule now: the list is drained before that chunk, whatever the remainder
    fixed = S.prefilter_model(fx.hashes, fx.needles, fx.thresh, rule="kernel")
    assert fixed.peak == (640 if remainder == 32 else ((remainder + 96) & 63) + 512) <= S.PEND_CAP


@pytest.mark.parametrize("k", range(4))
def test_chunk_position_builder_reaches_its_target(k):
    """a multi-lane chunk at group k of a step among one-lane groups: which drain rules overrun the list"""
    fx = S.BUILDERS[f"chunk_at_group{k}"]()
    peaks = {rule: S.prefilter_model(fx.hashes, fx.needles, fx.thresh, rule).peak for rule in S.RULES}
    assert peaks["kernel"] <= S.PEND_CAP
    assert (peaks["parent"] > S.PEND_CAP) == (k == 3) and (peaks["before_only"] > S.PEND_CAP) == (k < 3)


def test_kernel_drain_rule_bounds_every_group_order():
    """every sequence of four groups per step -- none, one lane with 1 or 32 registers, 2 / 16 / 17 / 64 lanes of 32 --
    entered with any remainder 0..63: the kernel's rule never holds more than the list's 640 descriptors, and never
    leaves more than 63 behind a step; the other two rules overrun on some order"""
    import itertools

    kinds = [[], [1], [32], [32] * 2, [32] * 16, [32] * 17, [32] * 64]
    worst = {rule: 0 for rule in S.RULES}
    for start in range(64):
        for seq in itertools.product(kinds, repeat=4):
            for rule in S.RULES:
                npend, peak = start, start
                for regs in seq:
                    if regs:
                        p, npend = S.group_pending(npend, regs, rule)
                        peak = max(peak, p)
                worst[rule] = max(worst[rule], peak)
                if rule == "kernel":
                    assert peak <= S.PEND_CAP, (start, seq)
                    assert (npend & 63 if npend >= 64 else npend) <= 63
    assert worst["kernel"] == S.PEND_CAP and worst["parent"] == 671 and worst["before_only"] > S.PEND_CAP


def test_replicated_peak_sits_in_both_workgroups_and_both_needle_chunks():
    fx = S.BUILDERS["peak_repl"]()
    m = S.prefilter_model(fx.hashes, fx.needles, fx.thresh)
    inst = m.instances()
    assert {w // 4 for w, _ in inst} == {0, 1} and {c for _, c in inst} == {0, 1}
    assert all(max(e.peak for e in evs) == 671 for evs in inst.values())


@pytest.mark.parametrize("name", list(S.BUILDERS))
def test_every_builder_meets_its_target(name):
    fx = S.BUILDERS[name]()  # (each builder asserts its target through the model)
    assert len(fx.hashes) == len(fx.ids) and fx.hashes.dtype == np.uint64 and fx.needles.dtype == np.uint64
    assert fx.target and len(S.reference_records(fx.hashes, fx.ids, fx.needles, fx.thresh, fx.masks)) > 0
    if fx.thresh <= 32:
        assert S.prefilter_model(fx.hashes, fx.needles, fx.thresh, rule="kernel").peak <= S.PEND_CAP


def test_model_counts_padding_candidates():
    # a lone last pair repeats itself in fields 2 and 3; padded slots / needles are hash 0
    h = np.array([1, 2, 1 << 40], np.uint64)
    q = np.array([3] * 65, np.uint64)
    m = S.prefilter_model(h, q, 3)
    assert m.pad_needle > 0 and m.pad_slot > 0


def _ref_via_oracle(orc, h, ids, q, thresh):
    out = []
    for j, t in enumerate(q.tolist()):
        oi, od = orc.scan64(h, ids, t, thresh)
        out += [(j << 39) | (int(d) << 32) | int(i) for i, d in zip(oi.tolist(), od.tolist())]
    return np.sort(np.array(out, np.uint64))


@pytest.mark.parametrize("thresh", [1, 4, 9, 64, 65])
def test_reference_agrees_with_the_oracle(orc, thresh):
    rng = np.random.default_rng(thresh)
    base = S._rand64(rng, 8)
    h = np.concatenate([S._near(rng, b, 30, 6) for b in base] + [np.array([0, 1, 3], np.uint64)])
    ids = np.arange(1, len(h) + 1, dtype=np.uint32)
    ids[::11] = 0
    q = np.concatenate([S._near(rng, b, 12, 5) for b in base] + [np.array([0, 2], np.uint64)])
    got = S.reference_records(h, ids, q, thresh)
    assert np.array_equal(got, _ref_via_oracle(orc, h, ids, q, thresh))


def test_reference_masks_and_multiset_diff():
    h = np.array([0b1010, 0b1000, 0b0010], np.uint64)
    q = np.array([0b1010, 0b1010], np.uint64)
    masks = np.array([0, 0b0010], np.uint64)
    r = S.unpack(S.reference_records(h, np.array([5, 6, 7], np.uint32), q, 3, masks))
    assert r.tolist() == [[0, 0, 5], [0, 1, 6], [0, 1, 7], [1, 0, 5], [1, 1, 7]]
    missing, extra = S.multiset_diff(np.array([1, 1, 2], np.uint64), np.array([1, 2, 2, 3], np.uint64))
    assert missing.tolist() == [2, 3] and extra.tolist() == [1]


def test_scan_mfma_knob_refuses_values_it_does_not_know():
    """"scan_mfma" outside 0..4 is refused and leaves the knob as it was (a test that means to force a kernel must not
    silently run another one)."""
    from cbird_amd import _lib

    L = _lib.lib()
    v = C.c_longlong(-99)
    try:
        for good in (0, 1, 2, 3, 4):
            assert L.cbh_set_tuning(b"scan_mfma", good) == _lib.CBH_OK
            assert L.cbh_get_tuning(b"scan_mfma", C.byref(v)) == _lib.CBH_OK and v.value == good
        for bad in (-1, 5, 7, 1 << 20):
            assert L.cbh_set_tuning(b"scan_mfma", bad) == _lib.CBH_E_INVAL
            assert L.cbh_get_tuning(b"scan_mfma", C.byref(v)) == _lib.CBH_OK and v.value == 4
    finally:
        L.cbh_set_tuning(b"scan_mfma", 1)


# ---- GPU: the full record multiset of every scan path -----------------------------------------------------------------
def _load(gpu, fx):
    idx = gpu.DctHashIndex()
    idx.load(fx.hashes, fx.ids)
    h, i = idx.download()  # a plain handle keeps load order: the layout the fixture aimed at is the one scanned
    assert np.array_equal(h, fx.hashes) and np.array_equal(i, fx.ids)
    return idx


def _scan(idx, needles, thresh, cap):
    import torch

    from cbird_amd import _lib

    L = _lib.lib()
    dq = torch.from_numpy(needles.view(np.int64)).cuda()
    drec = torch.zeros(max(1, cap), dtype=torch.int64, device="cuda")
    dtot = torch.zeros(1, dtype=torch.int64, device="cuda")
    _lib.check(L.cbh_idx64_scan_dev(idx.handle, dq.data_ptr(), len(needles), thresh, drec.data_ptr(), cap,
                                    dtot.data_ptr(), None), "scan")
    tot = int(dtot.item())
    return tot, np.sort(drec[:min(tot, cap)].cpu().numpy().view(np.uint64))


def _pre_mask():
    from cbird_amd import _lib

    v = C.c_longlong(0)
    assert _lib.lib().cbh_get_tuning(b"scan_pre_mask", C.byref(v)) == 0
    return v.value


def _assert_same(got, want, what):
    if np.array_equal(got, want):
        return
    missing, extra = S.multiset_diff(got, want)
    raise AssertionError(f"{what}: {len(got)} records, {len(want)} expected; {len(missing)} missing "
                         f"{S.unpack(missing[:4]).tolist()}, {len(extra)} extra {S.unpack(extra[:4]).tolist()}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_FIXTURES)
def test_scan_records_equal_the_reference(gpu, scan_path, name):
    fx = S.BUILDERS[name]()
    want = S.reference_records(fx.hashes, fx.ids, fx.needles, fx.thresh)
    idx = _load(gpu, fx)
    tot, got = _scan(idx, fx.needles, fx.thresh, 2 * len(want) + 4096)
    if fx.thresh < 64 and scan_path in ("mfma", "mfma_pre", "mfma_full"):
        took = (_pre_mask() >> fx.thresh) & 1
        if scan_path == "mfma_full":
            assert not took
        elif fx.prefilter:
            assert took, "the prefilter kernel did not take the launch"
    _assert_same(got, want, f"{name} on {scan_path}")
    assert tot == len(want), (name, scan_path, tot, len(want))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["removed_null_masked", "dense_field3_only", "chunk_at_group1"])
def test_masked_find_batch_equals_the_reference(gpu, scan_path, name):
    """find_batch(masks=...) (mask_ok in every kernel; the join does not take masked calls) with k = the largest count:
    every match of every needle in (score, mediaId) order -- with masks that cut some of the true matches."""
    fx = S.BUILDERS[name]()
    masks = fx.masks
    if masks is None:  # every other needle: the bits its near neighbours differ in mostly, so that some are cut
        masks = np.where(np.arange(len(fx.needles)) % 2 == 0, 0x0000FFFF0000FFFF, 0).astype(np.uint64)
    if name == "chunk_at_group1":  # (exact copies: a mask never cuts them -- flip bits of half the chunk's needles)
        fx = S.Fixture(fx.name, fx.hashes, fx.ids, fx.needles ^ np.where(np.arange(256) % 2 == 0, 1 << 3, 0).astype(
            np.uint64), fx.thresh)
    want = S.unpack(S.reference_records(fx.hashes, fx.ids, fx.needles, fx.thresh, masks))
    unmasked = S.reference_records(fx.hashes, fx.ids, fx.needles, fx.thresh)
    assert 0 < len(want) < len(unmasked)  # the masks exclude some matches and keep others
    counts = np.bincount(want[:, 0], minlength=len(fx.needles))
    k = int(counts.max())
    idx = _load(gpu, fx)
    gi, gs, gc = idx.find_batch(fx.needles, fx.thresh, k, masks=masks)
    assert gc.tolist() == counts.tolist()
    order = np.lexsort((want[:, 2], want[:, 1], want[:, 0]))
    w = want[order]
    starts = np.r_[0, np.cumsum(counts)]
    for j in np.nonzero(counts)[0].tolist():
        a, b = starts[j], starts[j + 1]
        assert gi[j, :b - a].tolist() == w[a:b, 2].tolist() and gs[j, :b - a].tolist() == w[a:b, 1].tolist(), j
        assert (gi[j, b - a:] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dense_all_fields", "peak_repl"])
def test_record_cap_below_the_total(gpu, scan_path, name):
    """a record buffer smaller than the answer: the total is exact, and what was stored is part of the answer"""
    fx = S.BUILDERS[name]()
    want = S.reference_records(fx.hashes, fx.ids, fx.needles, fx.thresh)
    idx = _load(gpu, fx)
    cap = len(want) // 3
    tot, got = _scan(idx, fx.needles, fx.thresh, cap)
    assert tot == len(want) and len(got) == cap
    missing, extra = S.multiset_diff(got, want)
    assert len(extra) == 0 and len(missing) == len(want) - cap


@pytest.mark.gpu
def test_join_on_a_wide_value_of_exact_duplicates(gpu):
    """"scan_mfma" 4 (the bucketed join wherever it can take the call): a chunk value with > 512 slots and > 2048 needles
    -- several jobs on both axes of the wide join -- made of exact duplicates that every chunk agrees on, at the
    thresholds of each join kernel (<= 4 by needle, 5 narrow, 6..8 wide); and the dense fixtures."""
    from cbird_amd import _lib

    L = _lib.lib()
    v = C.c_longlong(0)
    assert L.cbh_get_tuning(b"scan_joins", C.byref(v)) == 0
    joins0 = v.value
    fx = S.join_wide_value()
    runs = [(fx, t) for t in (4, 5, 6, 8)] + [(S.BUILDERS[k](), None) for k in
                                              ("dense_all_fields", "dense_field3_only", "peak_repl", "second_tile_only")]
    L.cbh_set_tuning(b"scan_mfma", 4)
    try:
        for f, t in runs:
            t = t or f.thresh
            want = S.reference_records(f.hashes, f.ids, f.needles, t)
            idx = _load(gpu, f)
            tot, got = _scan(idx, f.needles, t, len(want) + 4096)
            _assert_same(got, want, f"{f.name} t{t} on the join")
            assert tot == len(want), (f.name, t, tot, len(want))
    finally:
        L.cbh_set_tuning(b"scan_mfma", 1)
    assert L.cbh_get_tuning(b"scan_joins", C.byref(v)) == 0 and v.value - joins0 == len(runs)
