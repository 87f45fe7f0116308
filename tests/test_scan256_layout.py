"""The 256-bit scan on layout-aligned cases (tests/scan256_layout.py): fixtures that put matches at chosen workgroups,
waves, row tiles, registers, columns and fields of k_hamm256_mfma3 / k_hamm256_mfma / k_hamm256_small / k_hamm256_scan --
the packed accumulator over 2^24 and back, matches under the top field's carry, ragged and zero rows and needles, every
needle-count routing boundary, a record buffer that has to grow, a million rows through every prefetch slot -- and the
FULL sorted record list of every scan path against a plain reference, with the kernel that ran read back."""
import ctypes as C

import numpy as np
import pytest

import scan256_layout as S


def _id(case):
    name, p = case
    return f"{name}-{p[0]}-t{p[1]}" if isinstance(p, tuple) else f"{name}-{p}"


# ---- CPU: the model, the builders, the reference ------------------------------------------------------------------------
def test_register_rows_cover_each_tile_once():
    rows = sorted(int(S.reg_row(g, h)) for h in (0, 1) for g in range(16))
    assert rows == list(range(32))
    g, h = S.row_reg(np.arange(32))
    assert [int(S.reg_row(int(a), int(b))) for a, b in zip(g, h)] == list(range(32))


@pytest.mark.parametrize("case", S.CASES, ids=_id)
def test_every_builder_meets_its_target(case):
    fx = S.build(*case)  # (each builder asserts its target through the model)
    n, nq = len(fx.rows), len(fx.needles)
    assert fx.rows.dtype == np.uint8 and fx.rows.shape == (n, 32) and fx.needles.shape == (nq, 32) and fx.target
    p = fx.planted
    assert len(p) and (S.dist(fx.rows[p[:, 1]], fx.needles[p[:, 0]]) == p[:, 2]).all()
    assert (p[:, 2] < fx.thresh).any()
    for q0, q1 in fx.ranges():
        assert 0 <= q0 < q1 <= nq


def test_builders_are_seeded():
    a, b = S.carry_hidden(25), S.carry_hidden(25)
    assert np.array_equal(a.rows, b.rows) and np.array_equal(a.needles, b.needles)


def test_accumulator_model_invariants():
    """fields are 128 + b - d on the first 128 bits; a field without a tile keeps 64 + b; the end value is over 2^24
    exactly when field 2 is flagged; the partials of an exact copy rise by 16 2^(8 f) per block, and at threshold 25 pass
    2^24 inside the sixth MFMA (after the fifth: 2^23 + 88 * 65793 + 64 + 64 * 2^8 + 32 * 2^16 = 16 291 992)"""
    rng = np.random.default_rng(0)
    rows = S.rand_rows(rng, 200)
    trip = np.stack([np.stack([S.flip_in(rng, r, int(rng.integers(0, 100)), 0, 256) for _ in range(3)]) for r in rows])
    for thresh in (1, 17, 25, 40):
        st = S.accumulator_model(rows, trip, thresh)
        d = S.dist128(rows[:, None, :], trip)
        assert np.array_equal(st.fields, 128 + thresh - 1 - d)
        assert np.array_equal(st.end_ge, st.fields[:, 2] >= 128)
        st2 = S.accumulator_model(rows, trip, thresh, active=(True, False, False))
        assert (st2.fields[:, 1:] == 64 + thresh - 1).all() and not st2.end_ge.any()
    same = S.accumulator_model(rows[0], np.stack([rows[0]] * 3), 25)
    assert np.diff(same.partials).tolist() == [16] * 3 + [16 << 8] * 4 + [16 << 16] * 4
    assert same.end_ge and not same.mfma_ge and same.block_ge and same.fields.tolist() == [152, 152, 152]
    assert same.partials[9] == 16291992


def test_placement_restates_the_launch_arithmetic():
    # k_hamm256_small: 1.1 M rows fill the 2048-workgroup grid, tiles from 32768 on are the second trip
    L = S.launch_small(1_100_013, 512)
    assert (L["nt"], L["na"], L["group"], L["grid"], L["stride"]) == (16, 6, 3, 2048, 8192)
    p = S.place_small(np.array([0, 32 * 8192, 32 * 3 * 8192 + 33, 1 << 20, 1_100_012]), np.array([0, 33, 96, 500, 511]),
                      1_100_013, 512)
    assert p["u"].tolist() == [0, 1, 3, 0, 0] and p["trip"].tolist() == [0, 0, 0, 1, 1]
    assert p["acc"].tolist() == [0, 0, 1, 5, 5] and p["field"].tolist() == [0, 1, 0, 0, 0] and p["last_tile"].tolist()[-1]
    assert [S.launch_small(5003, q)["nt"] for q in (1, 128, 129, 256, 257, 512)] == [4, 4, 8, 8, 16, 16]
    assert [S.launch_small(5003, q)["group"] for q in (128, 256, 512)] == [2, 3, 3]
    # row-stationary kernels on 5003 rows: chunks shrink to 2 triples / 4 tiles / 256 needles
    assert S.launch_mfma3(5003, 1100) == dict(n_tiles=35, n_triples=12, wgs=4, tpc=2, chunks=6, pad_tiles=1)
    assert S.launch_mfma(5003, 1100) == dict(n_tiles=35, wgs=7, tpc=4, chunks=9, last_chunk_tiles=3)
    assert S.launch_scan(5003, 1100) == dict(tiles=3, q_chunk=256, chunks=5, last_chunk=76)
    # a large call keeps the full chunks
    assert S.launch_mfma3(10_000_000, 32_000)["tpc"] == 43 and S.launch_mfma(10_000_000, 32_000)["tpc"] == 128
    p3 = S.place_mfma3(np.array([1536 + 384 * 2 + 32 * 5 + 13]), np.array([96 * 3 + 64 + 7]), 5003, 1100)
    assert {k: int(v[0]) for k, v in p3.items()} == dict(wg=1, wave=2, tile=5, group=2, g=5, half=1, r=7, field=2, triple=3,
                                                         chunk=1)
    p1 = S.place_mfma(np.array([0, 0]), np.array([34 * 32, 33 * 32]), 5003, 1100)
    assert p1["tail"].tolist() == [True, False] and p1["second"].tolist() == [False, True]
    ps = S.place_scan(np.array([2048 + 256 * 3 + 9]), np.array([1099]), 5003, 1100)
    assert (int(ps["wg"][0]), int(ps["slot"][0]), int(ps["thread"][0]), int(ps["chunk"][0])) == (1, 3, 9, 4)


def test_needle_counts_reach_the_routing_boundaries():
    """which needle count of needle_shapes reaches which kernel, which padding and which tail of the two-tile loop"""
    n = 5003
    counts = S.NEEDLE_COUNTS
    small = {q: S.route(n, q, 25, "mfma") for q in counts}
    assert [q for q in counts if small[q] == S.K_SMALL4] == [1, 31, 32, 33, 64, 65, 95, 96, 97, 128]
    assert [q for q in counts if small[q] == S.K_SMALL8] == [129]
    assert [q for q in counts if small[q] == S.K_SMALL16] == [257, 258, 259, 512]
    assert [q for q in counts if small[q] == S.K_MFMA3] == [513, 1100]  # 512 descriptors is the last for k_hamm256_small
    rows = {q: S.route(n, q, 25, "mfma_rows") for q in counts}
    assert [q for q in counts if rows[q] == S.K_MFMA2] == [1, 31, 32, 33, 64]  # < 3 tiles: one tile per accumulator
    assert all(rows[q] == S.K_MFMA3 for q in counts if q > 64)
    assert all(S.route(n, q, 41, p) == S.K_MFMA4 for q in counts for p in ("mfma", "mfma_rows"))
    assert {S.launch_mfma3(n, q)["pad_tiles"] for q in counts if q > 64} == {0, 1, 2}  # whole and padded triples
    assert {S.launch_mfma3(n, q)["chunks"] for q in counts} >= {1, 2, 3, 6}
    tails = {S.launch_mfma(n, q)["last_chunk_tiles"] % 2 for q in counts}
    assert tails == {0, 1} and max(S.launch_mfma(n, q)["chunks"] for q in counts) == 9
    assert {q % 4 for q in counts} == {0, 1, 2, 3} and S.launch_scan(n, 1100)["chunks"] == 5
    # as shipped ("scan256_mfma" 1): the matrix cores from 64 needle descriptors and 4096 rows
    assert [S.route(n, q, 25, "mfma", forced=False) for q in (33, 64, 65)] == [S.K_SCAN, S.K_SMALL4, S.K_SMALL4]
    assert S.route(4095, 512, 25, "mfma", forced=False) == S.K_SCAN
    # thresholds around kPre128MaxThresh
    assert [S.route(n, 600, t, "mfma") for t in (39, 40, 41)] == [S.K_MFMA3, S.K_MFMA3, S.K_MFMA4]
    assert [S.route(n, 100, t, "mfma") for t in (39, 40, 41)] == [S.K_SMALL4, S.K_SMALL4, S.K_MFMA4]


@pytest.fixture(scope="module")
def cvo():
    from oracle import CvOracle

    return CvOracle()


@pytest.mark.parametrize("thresh", [1, 25, 41, 130, 257])
def test_reference_agrees_with_the_oracle_and_with_itself(cvo, thresh):
    rng = np.random.default_rng(thresh)
    rows = S.rand_rows(rng, 700)
    rows[5] = 0
    needles = np.stack([S.flip_in(rng, rows[int(rng.integers(0, 700))], int(rng.integers(0, 60)), 0, 256) for _ in range(90)])
    needles[3] = 0
    want = S.reference_records(rows, needles, thresh)
    assert np.array_equal(want, S.reference_records_matmul(rows, needles, thresh, chunk=128))
    r, d, c = cvo.knn(rows, needles, len(rows), thresh)
    wr, wd, wc = S.knn_from_records(want, len(needles), len(rows))
    assert np.array_equal(c, wc) and np.array_equal(r, wr) and np.array_equal(d, wd)
    assert len(want) == int(c.sum()) and (thresh != 257 or len(want) == 700 * 90)
    u = S.unpack(want)
    assert np.array_equal(S.pack_records(u[:, 0], u[:, 1], u[:, 2]), want)
    assert np.array_equal(S.below(want, 1), S.reference_records(rows, needles, 1))
    assert np.array_equal(S.restrict(want, 10, 50), S.reference_records(rows, needles[10:50], thresh))


def test_multiset_diff():
    missing, extra = S.multiset_diff(np.array([1, 1, 2], np.uint64), np.array([1, 2, 2, 3], np.uint64))
    assert missing.tolist() == [2, 3] and extra.tolist() == [1]


def test_soak_cases_are_seeded():
    a, b = S.soak_case(np.random.default_rng(5)), S.soak_case(np.random.default_rng(5))
    assert a["n"] == b["n"] == a["n_img"] * a["per"] and np.array_equal(a["queries"], b["queries"])
    assert a["queries"].shape == (a["nq"], 32) and np.array_equal(np.packbits(a["bits"], axis=1), a["queries"])


def test_scan256_knobs_refuse_values_they_do_not_know():
    """"scan256_mfma" outside 0..2 and "scan256_small" outside 0..1 are refused and leave the knob as it was (a test that
    means to force a kernel must not silently run another one); "scan256_kernels" is a read-back that only 0 clears."""
    from cbird_amd import _lib

    L = _lib.lib()
    v = C.c_longlong(-99)
    try:
        for good in (0, 1, 2):
            assert L.cbh_set_tuning(b"scan256_mfma", good) == _lib.CBH_OK
            assert L.cbh_get_tuning(b"scan256_mfma", C.byref(v)) == _lib.CBH_OK and v.value == good
        for bad in (-1, 3, 7, 1 << 20):
            assert L.cbh_set_tuning(b"scan256_mfma", bad) == _lib.CBH_E_INVAL
            assert L.cbh_get_tuning(b"scan256_mfma", C.byref(v)) == _lib.CBH_OK and v.value == 2
        for good in (1, 0):
            assert L.cbh_set_tuning(b"scan256_small", good) == _lib.CBH_OK
            assert L.cbh_get_tuning(b"scan256_small", C.byref(v)) == _lib.CBH_OK and v.value == good
        for bad in (-1, 2, 16, 1 << 20):
            assert L.cbh_set_tuning(b"scan256_small", bad) == _lib.CBH_E_INVAL
            assert L.cbh_get_tuning(b"scan256_small", C.byref(v)) == _lib.CBH_OK and v.value == 0
        assert L.cbh_set_tuning(b"scan256_kernels", 1) == _lib.CBH_E_INVAL
        assert L.cbh_set_tuning(b"scan256_kernels", 0) == _lib.CBH_OK
        assert L.cbh_get_tuning(b"scan256_kernels", C.byref(v)) == _lib.CBH_OK and v.value == 0
    finally:
        L.cbh_set_tuning(b"scan256_mfma", 1)
        L.cbh_set_tuning(b"scan256_small", 1)


# ---- GPU: the full sorted record list of every scan path ------------------------------------------------------------------
class _M:
    def __init__(self, id_, desc, path=""):
        self.id, self.keyPointDescriptors, self.path = id_, desc, path


def _index(rows, per_media=None, shards=None):
    from cbird_amd.cvfeatures import CvFeaturesIndex

    idx = CvFeaturesIndex(shards=shards)
    per = per_media or len(rows)
    idx.add([_M(i + 1, rows[a:a + per]) for i, a in enumerate(range(0, len(rows), per))])
    assert idx.count() == len(rows)
    return idx


def _kernels(clear=False):
    from cbird_amd import _lib

    v = C.c_longlong(-1)
    if clear:
        assert _lib.lib().cbh_set_tuning(b"scan256_kernels", 0) == 0
    assert _lib.lib().cbh_get_tuning(b"scan256_kernels", C.byref(v)) == 0
    return v.value


def _names(mask):
    return [name for bit, name in S.KERNEL_NAMES.items() if mask & bit]


def _assert_same(got, want, what):
    if np.array_equal(got, want):
        return
    missing, extra = S.multiset_diff(got, want)
    order = "" if len(missing) or len(extra) else " (the same records in another order)"
    raise AssertionError(f"{what}: {len(got)} records, {len(want)} expected; {len(missing)} missing (needle, distance, row) "
                         f"{S.unpack(missing[:4]).tolist()}, {len(extra)} extra {S.unpack(extra[:4]).tolist()}{order}")


_ref_cache = {}


def _reference(name, param, thresh=None):
    """the reference records of a fixture (the same for each scan path: computed once)"""
    key = (name, param, thresh)
    if key not in _ref_cache:
        fx = S.build(name, param)
        _ref_cache[key] = S.reference(fx.rows, fx.needles, thresh or fx.thresh)
    return _ref_cache[key]


def _radius(idx, needles, thresh, path, want, what, n=None):
    """radius_match(needles, thresh - 1) as records, in the order it returned them; asserts the kernel that ran, the list
    and the total"""
    _kernels(clear=True)
    m, first = idx.radius_match(needles, thresh - 1)
    ran = _kernels()
    kernel = S.route(idx.count() if n is None else n, len(needles), thresh, path)
    assert ran == kernel, f"{what}: aimed at {S.KERNEL_NAMES[kernel]}, ran {_names(ran)}"
    got = S.pack_records(m[:, 0], m[:, 2], m[:, 1].astype(np.uint32))
    print(f"{what}: {S.KERNEL_NAMES[kernel]}, {len(got)} records, {len(want)} expected")
    _assert_same(got, want, what)
    assert int(first[-1]) == len(m) == len(want), what
    assert np.array_equal(first, np.r_[0, np.cumsum(np.bincount(m[:, 0], minlength=len(needles)))])
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("case", S.SMALL_CASES, ids=_id)
def test_scan256_records_equal_the_reference(gpu, scan256_path, case):
    fx = S.build(*case)
    idx = _index(fx.rows)
    whole = _reference(*case)
    assert (S.unpack(whole)[:, 1] < fx.thresh).all() and len(whole) >= int((fx.planted[:, 2] < fx.thresh).sum()) > 0
    for q0, q1 in fx.ranges():
        want = S.restrict(whole, q0, q1)
        _radius(idx, fx.needles[q0:q1], fx.thresh, scan256_path, want, f"{fx.name}[{q0}:{q1}] on {scan256_path}")


@pytest.fixture(scope="module")
def streaming():
    """the 1.1 M rows, their index and the reference at the largest threshold, once per module"""
    fx = S.build("small_streaming", 1_100_013)
    return fx, _index(fx.rows), S.reference_records_matmul(fx.rows, fx.needles, 40)


@pytest.mark.gpu
@pytest.mark.parametrize("thresh,nq", [(25, 512), (40, 512), (40, 97), (25, 200)])
def test_small_streaming_records_equal_the_reference(gpu, scan256_path, streaming, thresh, nq):
    """k_hamm256_small<16> (and <4>, <8> with 97 and 200 needles) over 1.1 M rows: every prefetch slot, the second trip
    of the outer loop, the ragged last tile"""
    fx, idx, whole = streaming
    want = S.below(S.restrict(whole, 0, nq), thresh)
    assert len(want) >= nq * min(thresh, 40) // 40 - 1
    _radius(idx, fx.needles[:nq], thresh, scan256_path, want, f"{fx.name} t{thresh} q{nq} on {scan256_path}")


def _assert_knn(idx, needles, thresh, want, ks, what):
    for k in ks:
        gr, gd, gc = idx.knn(needles, k, thresh)
        wr, wd, wc = S.knn_from_records(want, len(needles), k)
        assert np.array_equal(gc, wc), (what, k)
        assert np.array_equal(gr, wr) and np.array_equal(gd, wd), (what, k)  # (distance, row) order, zeros past the count


@pytest.mark.gpu
@pytest.mark.parametrize("case,ks", [(("dense", 40), (3071, 3072, 3073)), (("carry_hidden", 25), (2, 3, 4)),
                                     (("real_zeros", 25), (3, 4, 5))], ids=["dense", "carry_hidden", "real_zeros"])
def test_knn_cut_at_below_and_above_the_count(gpu, scan256_path, case, ks):
    """knn with k below, at and above the per-needle count: ties by row, places past the count zero, counts exact"""
    fx = S.build(*case)
    want = _reference(*case)
    counts = np.bincount(S.unpack(want)[:, 0], minlength=len(fx.needles))
    assert int(counts.max()) == ks[1]
    idx = _index(fx.rows)
    _kernels(clear=True)
    _assert_knn(idx, fx.needles, fx.thresh, want, ks, f"{fx.name} on {scan256_path}")
    assert _kernels() == S.route(len(fx.rows), len(fx.needles), fx.thresh, scan256_path)


@pytest.mark.gpu
def test_records_are_unchanged_after_remove(gpu, scan256_path):
    """removal is a matter of the maps: the rows stay and still answer radius searches and take knn places"""
    fx = S.build("real_zeros", 25)
    want = _reference("real_zeros", 25)
    idx = _index(fx.rows, per_media=100)
    before = _radius(idx, fx.needles, fx.thresh, scan256_path, want, "before remove")
    idx.remove([1, 13])  # the media of the zero rows 3, 17 and of the last rows
    after = _radius(idx, fx.needles, fx.thresh, scan256_path, want, "after remove")
    assert np.array_equal(before, after) and idx.count() == len(fx.rows)
    _assert_knn(idx, fx.needles, fx.thresh, want, (4,), "knn after remove")


def _shard_stats(idx):
    from cbird_amd import _lib

    st = _lib.cbh_shard_stats()
    _lib.check(_lib.lib().cbh_idx256_shard_stats(idx.handle, C.byref(st)), "stats")
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("thresh", [40, 41])
def test_sharded_dense_grows_one_shards_block(gpu, scan256_path, thresh):
    """three shards: the 3072 rows sit on one of them, whose 2^22 / 3-record block overflows -- that shard alone scans
    again (rescans goes up), and the records are still the reference's"""
    fx = S.build("dense", thresh)
    want = _reference("dense", thresh)
    idx = _index(fx.rows, per_media=256, shards=(1, 3))
    assert sorted(idx.shard_rows()) == [0, 0, len(fx.rows)] and len(want) > (1 << 22) // 3
    s0 = _shard_stats(idx)
    _radius(idx, fx.needles, fx.thresh, scan256_path, want, f"sharded {fx.name} on {scan256_path}")
    s1 = _shard_stats(idx)
    assert s1.rescans > s0.rescans and s1.scans - s0.scans >= 2
    _assert_knn(idx, fx.needles[:64], fx.thresh, S.restrict(want, 0, 64), (10,), "sharded knn")


def _scan_stats(idx):
    from cbird_amd import _lib

    st = _lib.cbh_stats()
    _lib.check(_lib.lib().cbh_idx256_get_stats(idx.handle, C.byref(st)), "get_stats")
    return st


@pytest.mark.gpu
def test_statistics_of_a_scan_that_regrows(gpu):
    """what cbh_idx256_get_stats and cbh_idx256_shard_stats count of ONE radius search whose 4.7 M records outgrow the first
    block of 2^22 once.  A plain handle counts every attempt: 2 launches, 2 n nq pairs.  A sharded handle counts the call:
    1 launch, n nq pairs -- while its one shard with rows scanned twice (scans + 2, rescans + 1)."""
    from cbird_amd import _lib

    fx = S.build("dense", 40)
    n, nq = len(fx.rows), len(fx.needles)
    total = len(_reference("dense", 40))
    assert total > (1 << 22)
    out = np.zeros((total, 3), np.int32)
    first = np.zeros(nq + 1, np.uint64)
    for shards, launches, scans, rescans in ((None, 2, 0, 0), ((1, 3), 1, 2, 1)):
        idx = _index(fx.rows, per_media=256, shards=shards)
        a, s0 = _scan_stats(idx), _shard_stats(idx)
        _lib.check(_lib.lib().cbh_idx256_radius_match(idx.handle, fx.needles.ctypes.data, nq, fx.thresh - 1, out.ctypes.data,
                                                      total, first.ctypes.data), "radius_match")
        b, s1 = _scan_stats(idx), _shard_stats(idx)
        assert int(first[-1]) == total, shards
        assert b.scan_launches - a.scan_launches == launches, shards
        assert b.scan_pairs - a.scan_pairs == launches * n * nq, shards
        assert b.scan_ms > a.scan_ms, shards
        assert (s1.scans - s0.scans, s1.rescans - s0.rescans) == (scans, rescans), shards


@pytest.mark.gpu
@pytest.mark.parametrize("thresh,nq", [(25, 512), (40, 200), (41, 512)])
def test_sharded_segments_translate_rows(gpu, scan256_path, thresh, nq):
    """7 x 16 384 + 1000 rows added as media of 2048 rows over three shards: every shard holds more than one segment, and
    the planted matches lie on both sides of every segment border (k_rows_to_global)"""
    n = 7 * S.SHARD_RUN + 1000
    fx = S.build("small_streaming", n)
    assert {"border_lo", "border_hi", "last_tile"} <= set(fx.reached["classes"])
    rows_of = fx.planted[:, 1]
    assert set((rows_of[rows_of % S.SHARD_RUN == 0] // S.SHARD_RUN).tolist()) == set(range(1, 8))
    assert set(((rows_of[rows_of % S.SHARD_RUN == S.SHARD_RUN - 1] + 1) // S.SHARD_RUN).tolist()) == set(range(1, 8))
    idx = _index(fx.rows, per_media=2048, shards=(1, 3))
    st = _shard_stats(idx)
    per_shard = idx.shard_rows()
    assert st.shards == 3 and st.segments == 8 and min(per_shard) > S.SHARD_RUN and sum(per_shard) == n
    want = S.below(S.restrict(_reference("small_streaming", n, 41), 0, nq), thresh)
    # (every shard routes like the whole: forced paths do not look at the row count)
    assert len({S.route(m, nq, thresh, scan256_path) for m in per_shard + [n]}) == 1
    _radius(idx, fx.needles[:nq], thresh, scan256_path, want, f"sharded {fx.name} t{thresh} q{nq} on {scan256_path}")
    one = _index(fx.rows, per_media=2048)
    _radius(one, fx.needles[:nq], thresh, scan256_path, want, f"plain {fx.name} t{thresh} q{nq} on {scan256_path}")


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [33, 64, 65, 512, 513])
def test_shipped_routing_at_its_boundaries(gpu, nq):
    """"scan256_mfma" 1, the default no scan256_path value sets: the matrix cores from 64 needle descriptors and 4096 rows"""
    from cbird_amd import _lib

    assert _lib.lib().cbh_set_tuning(b"scan256_mfma", 1) == 0 and _lib.lib().cbh_set_tuning(b"scan256_small", 1) == 0
    for thresh in (25, 41):
        fx = S.needle_shapes(nq, thresh)
        want = S.reference(fx.rows, fx.needles, thresh)
        for rows in (fx.rows, fx.rows[:4095]):
            idx = _index(rows)
            _kernels(clear=True)
            m, first = idx.radius_match(fx.needles, thresh - 1)
            kernel = S.route(len(rows), nq, thresh, "mfma", forced=False)
            assert _kernels() == kernel, (nq, thresh, len(rows), _names(_kernels()))
            w = want[(want & np.uint64(0xFFFFFFFF)) < len(rows)]
            _assert_same(S.pack_records(m[:, 0], m[:, 2], m[:, 1].astype(np.uint32)), w, f"shipped routing q{nq} t{thresh}")


@pytest.mark.gpu
def test_seeded_soak_every_query(gpu, scan256_path):
    """a dozen cases of the soak's generator (tools/fuzz_scan256.py), every query of each against the plain reference"""
    rng = np.random.default_rng(2024)
    total = 0
    for c in range(12):
        case = S.soak_case(rng)
        rows, q, thresh = case["rows"], case["queries"], case["max_dist"] + 1
        want = _soak_reference(c, rows, q, thresh)
        idx = _index(rows, per_media=case["per"])
        _radius(idx, q, thresh, scan256_path, want, f"soak case {c} (n {case['n']}, nq {case['nq']}, thresh {thresh})")
        total += len(want)
    assert total > 1000


_soak_cache = {}


def _soak_reference(c, rows, q, thresh):
    if c not in _soak_cache:  # (the same cases on each path)
        _soak_cache[c] = S.reference(rows, q, thresh)
    return _soak_cache[c]
