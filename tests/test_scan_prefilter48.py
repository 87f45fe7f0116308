"""The 48-bit prefilter kernel (k_hamm64_mfma48, PRE48, cbird_amd/csrc/hamm64_mfma.hip) on the GPU, forced with
"scan_pre48" 1: the FULL record multiset of every case against the oracle AND against the same call on the three-field
kernel, and "scan_pre48_mask" says the kernel ran.  tests/scan48_layout.py restates the layout; the arithmetic on paper is
in tests/test_scan48_model.py.

Shapes: n = 1024 is one workgroup of the 8-tile kernels (4 waves x 8 tiles x 32 rows), 1024 + 37 and 3 x 1024 the ragged
and the several; the kernel as built keeps 6 tiles per wave, so 768 is its one workgroup and 1024 one and a third;
nq = 128 is one needle quadruple, 129 / 255 / 640 a lone pair behind one, a quadruple one needle short, five."""
import ctypes as C

import numpy as np
import pytest

import scan48_layout as M
import scan_layout as S

THRESHOLDS = (1, 7, 8, 16)
SHAPES = ((1024, 128), (1024 + 37, 129), (3 * 1024, 255), (1024, 640), (768, 128), (768 + 37, 255))
COMP = 0xFFFF0000FFFFFFFF  # flips every element of the 48-bit word (64-bit distance 48)


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
def lib48(gpu):
    """the matrix-core scan for any size, the 48-bit prefilter for every threshold it can represent"""
    from cbird_amd import _lib

    L = _lib.lib()
    _set(L, scan_mfma=2, scan_pre48=1)
    try:
        yield L
    finally:
        _set(L, scan_mfma=1, scan_pre48=-1, scan_mfma_pre_max=-1)


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


def _scan48(L, idx, needles, thresh, cap):
    out = _scan(L, idx, needles, thresh, cap)
    assert (_get(L, "scan_pre48_mask") >> thresh) & 1, "not the 48-bit prefilter kernel"
    assert not (_get(L, "scan_pre_mask") >> thresh) & 1, "a launch sets its bit in one of the two masks"
    return out


def _scan_full3(L, idx, needles, thresh, cap):
    _set(L, scan_pre48=0, scan_mfma_pre_max=0)
    try:
        out = _scan(L, idx, needles, thresh, cap)
        assert not (_get(L, "scan_pre48_mask") >> thresh) & 1 and not (_get(L, "scan_pre_mask") >> thresh) & 1
    finally:
        _set(L, scan_pre48=1, scan_mfma_pre_max=-1)
    return out


def oracle_records(orc, hashes, ids, needles, thresh):
    """sorted cbh_records needle << 39 | dist << 32 | id from the oracle's scan, needle by needle"""
    out = []
    for j, q in enumerate(np.asarray(needles, np.uint64).tolist()):
        oi, od = orc.scan64(hashes, ids, q, thresh)
        out.append((np.uint64(j) << np.uint64(39)) | (od.astype(np.uint64) << np.uint64(32)) | oi.astype(np.uint64))
    return np.sort(np.concatenate(out)) if out else np.zeros(0, np.uint64)


def _same(name, got, want):
    if not np.array_equal(got, want):
        missing, extra = S.multiset_diff(got, want)
        raise AssertionError(f"{name}: {len(got)} records, {len(want)} expected; {len(missing)} missing "
                             f"{S.unpack(missing[:4]).tolist()}, {len(extra)} extra {S.unpack(extra[:4]).tolist()}")


def _check(L, gpu, orc, name, hashes, ids, needles, thresh):
    want = oracle_records(orc, hashes, ids, needles, thresh)
    assert np.array_equal(want, S.reference_records(hashes, ids, needles, thresh))
    idx = _load(gpu, hashes, ids)
    cap = len(want) + 4096
    tot, got = _scan48(L, idx, needles, thresh, cap)
    _same(f"{name} t{thresh} vs oracle", got, want)
    assert tot == len(want)
    tot3, got3 = _scan_full3(L, idx, needles, thresh, cap)
    _same(f"{name} t{thresh} vs three-field kernel", got, got3)
    assert tot3 == tot
    return want


# ---- (a) the FP4 values the design rests on ----------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_fp4_value_table(gpu):
    """+-0.5 (the subnormal), +-1, +-4 under the block scales 2, 2^7, 2^10, 2^13, 2^19: one MFMA per code pair returns
    the exact product, for one element and for a sub-block of 16, in either K block"""
    from cbird_amd import _lib

    out = (C.c_float * 720)()
    _lib.check(_lib.lib().cbh_selftest_fp4_products(0, out), "fp4 products")
    got = np.frombuffer(out, np.float32).reshape(6, 6, 5, 2, 2)
    vals = np.array([0.5, -0.5, 1.0, -1.0, 4.0, -4.0])
    scales = np.array([2.0, 2.0 ** 7, 2.0 ** 10, 2.0 ** 13, 2.0 ** 19])
    cnt = np.array([1.0, 16.0])
    want = (vals[:, None, None, None, None] * vals[None, :, None, None, None] * scales[None, None, :, None, None]
            * cnt[None, None, None, :, None] * np.ones(2)[None, None, None, None, :])
    bad = np.argwhere(got != want.astype(np.float32))
    assert len(bad) == 0, [(b.tolist(), float(got[tuple(b)]), float(want[tuple(b)])) for b in bad[:8]]


# ---- (b) planted pairs ----------------------------------------------------------------------------------------------------
def planted(n, nq, thresh, seed):
    """t - 1 / t / t + 1 differing elements confined to one sub-block, in every field P Q R S (needle tile of its
    quadruple), every sub-block and on rows of both lane halves; unrelated hashes around them"""
    rng = np.random.default_rng(seed)
    slots, needles = S._rand64(rng, n), S._rand64(rng, nq)
    free = list(rng.permutation(nq).tolist())
    plan = []
    for field in range(4):
        for sb in range(3):
            for half in range(2):
                for d in (thresh - 1, thresh, thresh + 1):
                    if d > 16:
                        continue
                    j = next(x for x in free if (x // 32) % 4 == field)
                    free.remove(j)
                    row = int(rng.integers(0, n))
                    while ((row % 32) >> 2) & 1 != half:
                        row = int(rng.integers(0, n))
                    needles[j] = M.flip(slots[row], sb, d)
                    plan.append((j, d, row))
    return slots, np.arange(1, n + 1, dtype=np.uint32), needles, plan


@pytest.mark.gpu
@pytest.mark.parametrize("thresh", THRESHOLDS)
@pytest.mark.parametrize("n,nq", SHAPES)
def test_b_planted_pairs(gpu, orc, lib48, n, nq, thresh):
    slots, ids, needles, plan = planted(n, nq, thresh, 1000 * thresh + nq)
    want = {tuple(x) for x in S.unpack(_check(lib48, gpu, orc, f"planted n{n} nq{nq}", slots, ids, needles, thresh)).tolist()}
    for j, d, row in plan:
        assert ((j, d, row + 1) in want) == (d < thresh)
    assert len({(j // 32) % 4 for j, _, _ in plan}) == 4


# ---- (c) a field that borrows from the one above ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("thresh", THRESHOLDS)
def test_c_borrow_and_top_field_carry(gpu, orc, lib48, thresh):
    """same row, same column: the complement of the row's 48-bit word (h = 48) in field k, a needle at h = t - 1 in
    field k + 1 -- the match must survive the borrow; k = 2 is also the top field's carry (field 3 flagged), and a fourth
    case hides a match in field 0 behind that carry"""
    rng = np.random.default_rng(31 + thresh)
    n, nq = 1024 + 37, 640
    slots, needles = S._rand64(rng, n), S._rand64(rng, nq)
    want = []
    for quad, (k, lo_field) in enumerate(((0, None), (1, None), (2, None), (2, 0))):
        for half in range(2):
            row = int(rng.integers(0, n))
            while ((row % 32) >> 2) & 1 != half:
                row = int(rng.integers(0, n))
            c = int(rng.integers(0, 16)) + 16 * half
            H = int(slots[row])
            needles[128 * quad + 32 * k + c] = H ^ COMP
            needles[128 * quad + 32 * (k + 1) + c] = M.flip(H, 1, thresh - 1)
            want.append((128 * quad + 32 * (k + 1) + c, thresh - 1, row + 1))
            if lo_field is not None:
                needles[128 * quad + 32 * lo_field + c] = M.flip(H, 2, thresh - 1)
                want.append((128 * quad + 32 * lo_field + c, thresh - 1, row + 1))
    ids = np.arange(1, n + 1, dtype=np.uint32)
    got = {tuple(x) for x in S.unpack(_check(lib48, gpu, orc, "borrow", slots, ids, needles, thresh)).tolist()}
    assert set(want) <= got


# ---- (d) the pending list at its bound, (e) edge inputs --------------------------------------------------------------------
def _event_fixtures():
    from test_scan_prefilter_events import EVENT_FIXTURES

    return EVENT_FIXTURES


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["every_lane_t12", "every_lane_t16", "list_at_its_maximum", "carry_hides_a_match",
                                  "many_rows_one_needle"])
def test_d_pending_list(gpu, orc, lib48, name):
    """the duplicate groups of tests/test_scan_prefilter_events.py: equal hashes are candidates of any prefilter, so
    list_at_its_maximum leaves 63 descriptors and then adds one per lane of every group of a step here too"""
    fx = _event_fixtures()[name]()
    _check(lib48, gpu, orc, name, fx.hashes, fx.ids, fx.needles, fx.thresh)


@pytest.mark.gpu
@pytest.mark.parametrize("thresh", THRESHOLDS)
@pytest.mark.parametrize("name", ["removed_null_masked", "padding_385", "padding_769"])
def test_e_edge_inputs(gpu, orc, lib48, name, thresh):
    """slots of hash 0 and id 0, null and low-popcount needles, n and nq off every tile"""
    fx = S.BUILDERS[name]()
    _check(lib48, gpu, orc, name, fx.hashes, fx.ids, fx.needles, thresh)


@pytest.mark.gpu
@pytest.mark.parametrize("thresh", (7, 8))
def test_e_needle_masks(gpu, lib48, thresh):
    """find_batch(masks=...): a d_qmask call, mask_ok in the drain"""
    fx = S.BUILDERS["removed_null_masked"]()
    want = S.unpack(S.reference_records(fx.hashes, fx.ids, fx.needles, thresh, fx.masks))
    counts = np.bincount(want[:, 0], minlength=len(fx.needles))
    idx = _load(gpu, fx.hashes, fx.ids)
    gi, gs, gc = idx.find_batch(fx.needles, thresh, int(counts.max()), masks=fx.masks)
    assert (_get(lib48, "scan_pre48_mask") >> thresh) & 1
    assert gc.tolist() == counts.tolist()
    w = want[np.lexsort((want[:, 2], want[:, 1], want[:, 0]))]
    starts = np.r_[0, np.cumsum(counts)]
    for j in np.nonzero(counts)[0].tolist():
        a, b = starts[j], starts[j + 1]
        assert gi[j, :b - a].tolist() == w[a:b, 2].tolist() and gs[j, :b - a].tolist() == w[a:b, 1].tolist(), j


@pytest.mark.gpu
def test_e_keep_id0(gpu, orc, lib48):
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
    for thresh in (7, 8):
        p = gpu.SearchParams(dctThresh=thresh)
        for nd in media[:12:3]:
            got = idx.find_batch([nd], p)[0]
            assert (_get(lib48, "scan_pre48_mask") >> thresh) & 1
            wi, ws = orc.fdct_find(h, ids_after, np.array(nd.keyPointHashes, np.uint64), nd.id, thresh)
            assert [x.mediaId for x in got] == wi.tolist() and [x.score for x in got] == ws.tolist(), nd.id


# ---- (f) a sharded handle ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("thresh", THRESHOLDS)
def test_f_sharded_handle(gpu, orc, lib48, thresh):
    """three shards with ragged shares: one kernel choice and one needle expansion for the call"""
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
    assert (_get(lib48, "scan_pre48_mask") >> thresh) & 1
    wi, ws, wc = orc.find64_batch(slots, ids, needles, thresh, 8)
    assert (gc == wc).all() and (gi == wi).all() and (gs == ws).all()
    assert wc.sum() >= sum(d < thresh and ids[row] != 0 for _, d, row in plan)


# ---- (g) the route as shipped ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_g_default_routing(gpu):
    """2^31 pairs of unrelated hashes (65 536 slots x 32 768 needles) are probed.  The model -- the routing comment in
    hamm64_scan.hip -- gives the 48-bit prefilter 14.0 + 2.8e4 x 2.0e-6 = 14.06 ms per 10^12 pairs at both thresholds
    (P[Bin(48, 1/2) <= t or > 32 + t] = 2.0e-6), the 32-bit prefilter 8.55 + 2.4e4 x r_cand = 15.0 at 7 (r_cand 2.68e-4)
    and 33.6 at 8 (1.05e-3), the three-field kernel 15.75: threshold 7 stays on the 32-bit prefilter (14.06 is not below
    0.9 x 15.0), threshold 8 takes the 48-bit one.  The records equal the three-field kernel's."""
    from cbird_amd import _lib

    L = _lib.lib()
    rng = np.random.default_rng(99)
    n, nq = 65536, 32768
    slots, needles = S._rand64(rng, n), S._rand64(rng, nq)
    for j in range(0, 64):  # a few true matches, so that the record sets are not empty
        needles[j * 512 + j] = S._near(rng, slots[j * 1000 + 3], 1, 6)[0]
    ids = np.arange(1, n + 1, dtype=np.uint32)
    idx = _load(gpu, slots, ids)
    for thresh, want48 in ((7, False), (8, True)):
        probes = _get(L, "scan_probes")
        tot, got = _scan(L, idx, needles, thresh, 1 << 16)
        assert _get(L, "scan_probes") == probes + 1
        r48 = _get(L, "scan_probe_rate48_e9") * 1e-9
        assert r48 < 2e-5, r48
        assert bool((_get(L, "scan_pre48_mask") >> thresh) & 1) == want48
        assert bool((_get(L, "scan_pre_mask") >> thresh) & 1) == (not want48)
        _set(L, scan_pre48=0, scan_mfma_pre_max=0)
        try:
            tot3, got3 = _scan(L, idx, needles, thresh, 1 << 16)
        finally:
            _set(L, scan_pre48=-1, scan_mfma_pre_max=-1)
        assert tot == tot3 >= 32
        _same(f"default route t{thresh}", got, got3)
