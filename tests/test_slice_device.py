"""Index::slice() (the device routes of cbird_amd/csrc/slice.hip, and cbh_idx64_slice, which still goes through the
host and whose results any later route has to keep): cbh_idx64_slice, cbh_idx256_slice, cbh_color_slice and
cbh_vidx_slice against what the library already produces -- np.isin on the downloaded parent for the 64-bit index, the
rows_of + download_rows + add composition for the 256-bit one, add of the kept subset for colour, add_video for video --
bit for bit, on the plain handle and on sharded ones (five and three logical shards; under tests/shim/vdev.c, where
tests/test_slice_virtual_devices.py runs this file again, a sparse mask of three ordinals and 2 ordinals x 2 shards, so
that the copies between ordinals execute).

Sizes of the 64-bit cases: 2048 and 2048 * 2048 slots are where a device route in tiles of 2048 slots, with a scan of
2048 tile counts per workgroup, has its block and level boundaries; one size on each side of both."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_VDEV = int(os.environ.get("CBH_VDEV", "0"))
# (device_mask, shards_per_device); None = the plain one-device handle
SHAPES = {"mask1101": (0b1101, 1), "dev2x2": (0x3, 2)} if _VDEV > 1 else {"one": None, "shards5": (1, 5), "shards3": (1, 3)}
SHARDED = {k: v for k, v in SHAPES.items() if v is not None}
N64 = [0, 1, 255, 256, 257, 2047, 2048, 2049, 4097, 70001, 2048 * 2048, 2048 * 2048 + 1]


def _tuning(L, key):
    v = C.c_longlong(-2)
    assert L.cbh_get_tuning(key, C.byref(v)) == 0, key
    return int(v.value)


def _p(a):
    return a.ctypes.data if len(a) else None


def _shim_stats():
    """under tests/shim/vdev.c: (copies between ordinals, kernels sent to a stream of an ordinal that was not current,
    events recorded on another ordinal's stream) so far; None without the shim"""
    if _VDEV <= 1:
        return None
    shim = C.CDLL(None)
    shim.vdev_stat.restype = C.c_long
    return shim.vdev_stat(1), shim.vdev_stat(4), shim.vdev_stat(5)


def _ordinals_were_crossed_in_order(before):
    if before is not None:
        after = _shim_stats()
        assert after[0] > before[0] and after[1] == 0 and after[2] == 0, (before, after)


# ---- 64-bit index -----------------------------------------------------------------------------------------------------
def _build64(gpu, L, n, shape, seed):
    """n slots whose ids repeat 1-7 times (a DctFeaturesIndex), loaded in one load and two adds, some ids removed with
    their hashes and some ids only -> (index, hashes, ids as downloaded)"""
    rng = np.random.default_rng(seed)
    ids = np.repeat(np.arange(1, n + 2, dtype=np.uint32), rng.integers(1, 8, n + 1))[:n].copy()
    h = rng.integers(1, 1 << 63, n, dtype=np.uint64)
    if n > 8:  # near-duplicates, so that a threshold search has something to find
        dup = rng.integers(0, n, n // 8)
        h[dup] = h[rng.integers(0, n, n // 8)] ^ (np.uint64(1) << rng.integers(0, 63, n // 8).astype(np.uint64))
    idx = gpu.DctHashIndex(shards=shape) if shape else gpu.DctHashIndex()
    a, b = n * 6 // 10, n * 85 // 100
    assert L.cbh_idx64_load(idx.handle, _p(h[:a]), _p(ids[:a]), a) == 0
    assert L.cbh_idx64_add(idx.handle, _p(h[a:b]), _p(ids[a:b]), b - a) == 0
    assert L.cbh_idx64_add(idx.handle, _p(h[b:]), _p(ids[b:]), n - b) == 0
    if n:
        uniq = np.unique(ids)
        rm = np.ascontiguousarray(rng.choice(uniq, max(1, len(uniq) // 10), replace=False), np.uint32)
        rm2 = np.ascontiguousarray(rng.choice(uniq, max(1, len(uniq) // 10), replace=False), np.uint32)
        assert L.cbh_idx64_remove(idx.handle, rm.ctypes.data, len(rm)) == 0
        assert L.cbh_idx64_remove_ids_only(idx.handle, rm2.ctypes.data, len(rm2)) == 0
    ph, pi = idx.download()
    assert len(pi) == n
    return idx, ph, pi


def _wanted64(pi, n, rng):
    uniq = np.unique(pi[pi != 0]) if n else np.zeros(0, np.uint32)
    some = rng.choice(uniq, len(uniq) * 4 // 10, replace=False) if len(uniq) else uniq
    lacking = np.array([n + 100, n + 101, 0xfffffff0], np.uint32)
    mixed = np.concatenate([some, some[: len(some) // 3], lacking]).astype(np.uint32)
    rng.shuffle(mixed)
    return {"some": mixed, "all": uniq.astype(np.uint32), "none": lacking, "empty": np.zeros(0, np.uint32),
            "with0": np.concatenate([some[: len(some) // 2], [0]]).astype(np.uint32)}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("n", N64)
def test_idx64_slice_equals_isin_on_the_parent(gpu, orc, n, shape):
    from cbird_amd import _lib

    L = _lib.lib()
    idx, ph, pi = _build64(gpu, L, n, SHAPES[shape], seed=n % 1000 + 7)
    rng = np.random.default_rng(n + 1)
    for name, want in _wanted64(pi, n, rng).items():
        keep = np.isin(pi, want)
        eh, ei = ph[keep], pi[keep]
        h = L.cbh_idx64_slice(idx.handle, _p(want), len(want))
        assert h, (name, L.cbh_last_error())
        sl = gpu.DctHashIndex(_handle=h)
        assert sl.isLoaded() and sl.count() == len(ei), name
        gh, gi = sl.download()
        assert (gi == ei).all() and (gh == eh).all(), name
        R, m = idx.shard_count(), len(ei)
        assert sl.shard_count() == R
        assert sl.shard_counts() == [(s + 1) * m // R - s * m // R for s in range(R)], name
        if name == "with0" and n:
            assert (ei == 0).any()  # removed slots were kept
        if name in ("some", "with0"):
            q = np.concatenate([eh[:: max(1, m // 48)][:48], rng.integers(1, 1 << 63, 16, dtype=np.uint64)])
            fi, fs, fc = sl.find_batch(q, 5, 8)
            if m:
                wi, ws, wc = orc.find64_batch(eh, ei, q, 5, 8)
                assert (fc == wc).all() and (fi == wi).all() and (fs == ws).all(), name
            else:
                assert not fc.any()


# ---- 256-bit index ----------------------------------------------------------------------------------------------------
def _idx256(shape):
    from cbird_amd.cvfeatures import CvFeaturesIndex

    return CvFeaturesIndex(shards=shape) if shape else CvFeaturesIndex()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_idx256_slice_equals_todays_composition(gpu, shape):
    from cbird_amd import _lib
    from cbird_amd.cvfeatures import CvFeaturesIndex

    L = _lib.lib()
    rng = np.random.default_rng(31)
    sharded = SHAPES[shape] is not None
    mids = (np.arange(160) * 3 + 5).astype(np.uint32)
    counts = np.full(160, 700) if sharded else rng.integers(1, 701, 160)  # 700: runs of 16384 rows are crossed
    rows = rng.integers(0, 256, (int(counts.sum()), 32), dtype=np.uint8)
    first = np.concatenate([[0], np.cumsum(counts)])
    idx = _idx256(SHAPES[shape])
    for i, mid in enumerate(mids):
        r = rows[first[i]:first[i + 1]]
        assert L.cbh_idx256_add(idx.handle, int(mid), r.ctypes.data, len(r)) == 0
    removed = np.array([mids[3], mids[101]], np.uint32)
    idx.remove(removed)
    absent = np.array([1, 4000], np.uint32)
    want = np.concatenate([mids[::2], removed, absent, mids[:20:2]]).astype(np.uint32)
    rng.shuffle(want)
    # today's composition: rows_of + download_rows + add, in ascending id
    exp = _idx256(SHAPES[shape])
    for mid in sorted(set(int(x) for x in want)):
        d = idx.descriptorsForMediaId(mid)
        if len(d):
            assert L.cbh_idx256_add(exp.handle, mid, d.ctypes.data, len(d)) == 0
    s0, shim0 = _tuning(L, b"slices_on_device"), _shim_stats()
    h = L.cbh_idx256_slice(idx.handle, want.ctypes.data, len(want))
    assert h, L.cbh_last_error()
    _ordinals_were_crossed_in_order(shim0)  # (half of the media: the shards fill differently, rows change ordinal)
    sl = CvFeaturesIndex(_handle=h)
    assert _tuning(L, b"slices_on_device") == s0 + 1
    assert sl.count() == exp.count() > 0 and sl.isLoaded()
    f, c, f2, c2 = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    for mid in list(mids) + list(absent):
        assert L.cbh_idx256_rows_of(sl.handle, int(mid), C.byref(f), C.byref(c)) == 0
        assert L.cbh_idx256_rows_of(exp.handle, int(mid), C.byref(f2), C.byref(c2)) == 0
        assert (f.value, c.value) == (f2.value, c2.value), mid
    got, wantrows = np.zeros((sl.count(), 32), np.uint8), np.zeros((exp.count(), 32), np.uint8)
    assert L.cbh_idx256_download_rows(sl.handle, 0, sl.count(), got.ctypes.data) == 0
    assert L.cbh_idx256_download_rows(exp.handle, 0, exp.count(), wantrows.ctypes.data) == 0
    assert (got == wantrows).all()
    assert sl.shard_rows() == exp.shard_rows() and len(sl.shard_rows()) == len(idx.shard_rows())
    q = rows[rng.integers(0, len(rows), 200)].copy()
    q[::3, 7] ^= 0x5a
    for a, b in zip(sl.knn(q, 10, 30), exp.knn(q, 10, 30)):
        assert (np.asarray(a) == np.asarray(b)).all()
    assert sl.knn(q, 10, 30)[2].sum() > 0
    # the parent is as it was
    assert idx.count() == len(rows) and (idx.descriptorsForMediaId(int(mids[7])) == rows[first[7]:first[8]]).all()


# ---- colour -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 255, 4097])
def test_color_slice_equals_add_of_the_kept_subset(gpu, n):
    from cbird_amd import _lib
    from cbird_amd.colordesc import COLOR_DTYPE, ColorDescIndex
    from oracle import ColorOracle
    from test_color import synth_descriptors

    L = _lib.lib()
    co = ColorOracle()
    descs, ids = synth_descriptors(n, 17 + n)
    needles, _ = synth_descriptors(40, 99)
    needles = needles[needles["numColors"] > 0][:6]
    assert len(needles) == 6
    idx = ColorDescIndex()
    assert L.cbh_color_add(idx.handle, ids.ctypes.data, descs.ctypes.data, n) == 0
    if n >= 7:
        idx.remove([int(ids[1]), int(ids[n // 2])])  # two entries removed: id 0, cleared descriptor
    pi, pd = np.zeros(n, np.uint32), np.zeros(n, COLOR_DTYPE)
    assert L.cbh_color_download(idx.handle, pi.ctypes.data, pd.ctypes.data, n) == 0
    # odd and even numbers of kept entries (3 and 4 of 7, 128 and 129 of 255), the very last entry always among them; a
    # third list also keeps the removed ones
    last = int(ids[-1])
    live = [int(i) for i in pi if i and i != last]
    k = 3 if n == 7 else n // 2 + 1
    wants = [live[: k - 1] + [last], live[:k] + [last, last, 10 ** 6], live[: k - 1] + [last, 0]]
    seen = set()
    for want in wants:
        w = np.array(want, np.uint32)
        keep = np.isin(pi, w)
        if 0 not in want:
            seen.add(int(keep.sum()) % 2)
        exp = ColorDescIndex()
        ki, kd = np.ascontiguousarray(pi[keep]), np.ascontiguousarray(pd[keep])
        assert L.cbh_color_add(exp.handle, ki.ctypes.data, kd.ctypes.data, len(ki)) == 0
        s0 = _tuning(L, b"slices_on_device")
        h = L.cbh_color_slice(idx.handle, w.ctypes.data, len(w))
        assert h, L.cbh_last_error()
        sl = ColorDescIndex(_handle=h)
        assert _tuning(L, b"slices_on_device") == s0 + 1
        m = int(keep.sum())
        assert sl.count() == exp.count() == m and keep[-1]
        gi, gd = np.zeros(m, np.uint32), np.zeros(m, COLOR_DTYPE)
        assert L.cbh_color_download(sl.handle, gi.ctypes.data, gd.ctypes.data, m) == 0
        assert gi.tobytes() == ki.tobytes() and gd.tobytes() == kd.tobytes()
        assert sl.distances(needles).tobytes() == exp.distances(needles).tobytes()
        for t in needles:
            class M:
                id, path, colorDescriptor = 0, "", t
            oi, osc = co.find(kd, ki, t)
            assert [(x.mediaId, x.score) for x in sl.find(M)] == list(zip(oi.tolist(), osc.tolist()))
    assert n == 1 or seen == {0, 1}


@pytest.mark.parametrize("n,kept", [(7, 3), (255, 128)])
def test_color_slice_can_be_added_to(gpu, n, kept):
    """a slice's planes are allocated to fit (capacity = kept rounded up to 4), not by add()'s growth path: a later add
    first lands in that slack, on the padding entry (3 of 7 kept: capacity 4), or has none and must grow (128 of 255),
    then grows again; after each the slice equals an index that was filled by add() alone"""
    from cbird_amd import _lib
    from cbird_amd.colordesc import COLOR_DTYPE, ColorDescIndex
    from test_color import synth_descriptors

    L = _lib.lib()
    descs, ids = synth_descriptors(n, 17 + n)
    more, _ = synth_descriptors(8, 5)
    more_ids = np.arange(9001, 9009, dtype=np.uint32)
    needles, _ = synth_descriptors(40, 99)
    needles = needles[needles["numColors"] > 0][:6]
    idx, exp = ColorDescIndex(), ColorDescIndex()
    assert L.cbh_color_add(idx.handle, ids.ctypes.data, descs.ctypes.data, n) == 0
    want = np.ascontiguousarray(ids[-kept:])
    assert L.cbh_color_add(exp.handle, want.ctypes.data, np.ascontiguousarray(descs[-kept:]).ctypes.data, kept) == 0
    h = L.cbh_color_slice(idx.handle, want.ctypes.data, kept)
    assert h, L.cbh_last_error()
    sl = ColorDescIndex(_handle=h)
    m = kept
    for a, b in ((0, 1), (1, 8)):
        for ix in (sl, exp):
            assert L.cbh_color_add(ix.handle, more_ids[a:b].ctypes.data, np.ascontiguousarray(more[a:b]).ctypes.data, b - a) == 0
        m += b - a
        got = []
        for ix in (sl, exp):
            assert ix.count() == m
            gi, gd = np.zeros(m, np.uint32), np.zeros(m, COLOR_DTYPE)
            assert L.cbh_color_download(ix.handle, gi.ctypes.data, gd.ctypes.data, m) == 0
            got.append((gi.tobytes(), gd.tobytes(), ix.distances(needles).tobytes()))
        assert got[0] == got[1], (n, m)


# ---- video ------------------------------------------------------------------------------------------------------------
_VSHAPES = {k: v for k, v in SHAPES.items() if k in ("one", "shards3", "mask1101", "dev2x2")}


@pytest.mark.parametrize("radix", [0, 10])
@pytest.mark.parametrize("shape", list(_VSHAPES))
def test_vidx_slice_equals_add_video_of_the_same_videos(gpu, shape, radix):
    from cbird_amd import _lib, synth_video
    from cbird_amd._lib import cbh_vmatch
    from cbird_amd.video import DctVideoIndex

    L = _lib.lib()
    clips = synth_video.make_clips(40, 60, seed=9, subclip_frac=0.3, max_gap=5)
    vids = [(np.ascontiguousarray(f, np.int32), np.ascontiguousarray(h, np.uint64)) for f, h in clips]

    def add(ix, k):
        f, h = vids[k]
        assert L.cbh_vidx_add_video(ix.handle, k + 1, f.ctypes.data, h.ctypes.data, len(f)) == 0

    full = DctVideoIndex(shards=_VSHAPES[shape]) if _VSHAPES[shape] else DctVideoIndex()
    for k in range(40):
        add(full, k)
    assert L.cbh_vidx_set_radix(full.handle, radix) == 0
    rng = np.random.default_rng(3)
    order = [int(x) + 1 for x in rng.permutation(40)[:15]]
    want = np.array(order[:6] + [777] + order[6:] + [order[2]], np.uint32)  # one absent id, one repeated
    exp = DctVideoIndex(shards=_VSHAPES[shape]) if _VSHAPES[shape] else DctVideoIndex()
    for mid in order:
        add(exp, mid - 1)
    assert L.cbh_vidx_set_radix(exp.handle, radix) == 0
    h = L.cbh_vidx_slice(full.handle, want.ctypes.data, len(want))
    assert h, L.cbh_last_error()
    sl = DctVideoIndex(_handle=h)
    assert sl.count() == exp.count() == 15

    def find_video(ix, k):
        f, hh = vids[k]
        out, n = (cbh_vmatch * 64)(), C.c_size_t(0)
        assert L.cbh_vidx_find_video(ix.handle, f.ctypes.data, hh.ctypes.data, len(f), 0, 5, 0, 5, 30, 0, out, 64, C.byref(n)) == 0
        return [(out[i].id, out[i].score, out[i].src_in, out[i].dst_in, out[i].len) for i in range(n.value)]

    def find_frame(ix, hash_):
        out, n = (cbh_vmatch * 256)(), C.c_size_t(0)
        assert L.cbh_vidx_find_frame(ix.handle, int(hash_), 6, 0, 0, out, 256, C.byref(n)) == 0
        return [(out[i].id, out[i].score, out[i].src_in, out[i].dst_in, out[i].len) for i in range(n.value)]

    found = 0
    for k in [order[0] - 1, order[5] - 1, order[14] - 1, 38, 39]:
        a, b = find_video(sl, k), find_video(exp, k)
        assert a == b, k
        found += len(a)
    for k in [order[1] - 1, order[7] - 1, order[9] - 1, 0, 37]:
        a, b = find_frame(sl, vids[k][1][len(vids[k][1]) // 2]), find_frame(exp, vids[k][1][len(vids[k][1]) // 2])
        assert a == b, k
        found += len(a)
    assert found > 0
    assert L.cbh_vidx_entries(sl.handle, 0) == L.cbh_vidx_entries(exp.handle, 0) > 0


# ---- refused allocations ----------------------------------------------------------------------------------------------
def _slice_case(gpu, name):
    """-> (slice call returning a raw handle or None, destroy, check that the parent still answers, the parent)"""
    from cbird_amd import _lib
    from cbird_amd.colordesc import ColorDescIndex
    from test_color import synth_descriptors

    L = _lib.lib()
    rng = np.random.default_rng(5)
    shape = list(SHARDED.values())[-1] if name.endswith("_sharded") else None
    if name.startswith("idx256"):
        cv = _idx256(shape)
        rows = rng.integers(0, 256, (60 * 700, 32), dtype=np.uint8)
        for i in range(60):
            assert L.cbh_idx256_add(cv.handle, i + 1, rows[i * 700:(i + 1) * 700].ctypes.data, 700) == 0
        want = np.arange(1, 61, 2, dtype=np.uint32)
        q = rows[::211][:100].copy()
        ref = cv.knn(q, 6, 30)
        return (lambda: L.cbh_idx256_slice(cv.handle, want.ctypes.data, len(want)), L.cbh_idx256_destroy,
                lambda: all((np.asarray(a) == np.asarray(b)).all() for a, b in zip(cv.knn(q, 6, 30), ref)), cv)
    cd, cids = synth_descriptors(3000, 8)
    col = ColorDescIndex()
    assert L.cbh_color_add(col.handle, cids.ctypes.data, cd.ctypes.data, len(cids)) == 0
    cwant = np.ascontiguousarray(cids[::2])
    cref = col.find_batch(cd[:8], 5)
    return (lambda: L.cbh_color_slice(col.handle, cwant.ctypes.data, len(cwant)), L.cbh_color_destroy,
            lambda: all((a == b).all() for a, b in zip(col.find_batch(cd[:8], 5), cref)), col)


@pytest.mark.parametrize("name", ["idx256", "idx256_sharded", "color"])
def test_every_allocation_of_a_slice_may_be_refused(gpu, name):
    """tests/test_error_paths.py's walk over one call of each slice entry point: "fault_alloc_after" 0, 1, 2, ... until
    the call makes fewer allocations than that.  Every refused call returns NULL with CBH_E_NOMEM, leaves no arena block
    handed out, and the parent still answers"""
    from cbird_amd import _lib

    L = _lib.lib()
    call, destroy, parent_ok, _parent = _slice_case(gpu, name)
    h = call()  # (one-time costs -- code objects, workspaces of the parent -- are not part of the walk)
    assert h
    destroy(h)
    assert parent_ok()
    refused = 0
    for k in range(200):
        live0 = _tuning(L, b"arena_live_bytes")
        fired0 = _tuning(L, b"fault_fired")
        L.cbh_set_tuning(b"fault_alloc_after", k)
        try:
            h = call()
            code = L.cbh_last_error_code()
        finally:
            L.cbh_set_tuning(b"fault_alloc_after", -1)
        if _tuning(L, b"fault_fired") == fired0:
            assert h, "the call failed although no allocation was refused"
            destroy(h)
            break
        refused += 1
        assert not h and code == _lib.CBH_E_NOMEM, (k, h, code)
        assert _tuning(L, b"arena_live_bytes") == live0, k
        assert parent_ok(), k
    else:
        pytest.fail("the call never ran out of allocations to refuse")
    assert refused >= 1
    print(f"{name}: {refused} allocations refused once each")


def test_vidx_slice_allocates_nothing_on_the_device(gpu):
    """cbh_vidx_slice is host code: with the next device allocation armed to fail it succeeds and the gate stays armed"""
    from cbird_amd import _lib
    from cbird_amd.video import DctVideoIndex

    L = _lib.lib()
    v = DctVideoIndex()
    f, h = np.arange(5, dtype=np.int32), np.arange(11, 16, dtype=np.uint64)
    assert L.cbh_vidx_add_video(v.handle, 4, f.ctypes.data, h.ctypes.data, 5) == 0
    want = np.array([4], np.uint32)
    L.cbh_set_tuning(b"fault_alloc_after", 0)
    try:
        s = L.cbh_vidx_slice(v.handle, want.ctypes.data, 1)
        assert s and _tuning(L, b"fault_alloc_after") == 0
        assert L.cbh_vidx_count(s) == 1
        L.cbh_vidx_destroy(s)
    finally:
        L.cbh_set_tuning(b"fault_alloc_after", -1)
