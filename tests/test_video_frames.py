"""Image needles of the video index in batches (cbh_vidx_find_frames_batch, cbird_amd/csrc/frames.hip): findFrame
(src/dctvideoindex.cpp:291-387) for a needle batch with one scan and one reduction on the device, searchIndex over it,
and the coalesced single-needle entry.  Held against the real RadixMap's committed answers, the single-needle
cbh_vidx_find_frame, the oracle, and literal rows for the run shapes at which the per-run reduction can go wrong."""
import ctypes as C
import threading
import warnings

import numpy as np
import pytest

from conftest import load_golden

H = 0x0F0F0F0F0F0F0F0E  # 31 ones, bit 0 clear


@pytest.fixture(scope="module")
def vorc():
    from oracle import VideoOracle

    return VideoOracle()


class _M:
    """an image needle: no videoIndex"""

    def __init__(self, mid, dct_hash, src_in=-1, path=""):
        from cbird_amd.index import MatchRange

        self.id, self.dctHash, self.path = int(mid), int(dct_hash), path or f"n{mid}"
        self.matchRange = MatchRange(dstIn=int(src_in))
        self.score = -1

    def isValid(self):
        return True


def _rows(matches):
    return [(x.mediaId, x.score, x.range.srcIn, x.range.dstIn, x.range.len) for x in matches]


def _video_media(clips, ids):
    from cbird_amd.video import VideoIndex

    media = []
    for mid, (f, h) in zip(ids, clips):
        m = _M(mid, 0, path=f"v{mid}")
        m.videoIndex = VideoIndex([int(x) for x in f], [int(x) for x in h])
        media.append(m)
    return media


def _raw_batch(L, handle, hashes, src_in, thresh, skip, cap):
    """cbh_vidx_find_frames_batch as it is -> (rc, per-needle row lists or None, out_offsets)"""
    hs = np.ascontiguousarray(hashes, np.uint64)
    si = None if src_in is None else np.ascontiguousarray(src_in, np.int32)
    offs = np.zeros(len(hs) + 1, np.uint64)
    from cbird_amd import _lib

    buf = (_lib.cbh_vmatch * max(1, cap))()
    rc = L.cbh_vidx_find_frames_batch(handle, hs.ctypes.data, None if si is None else si.ctypes.data, len(hs), thresh, skip,
                                      buf, cap, offs.ctypes.data)
    rows = None
    if rc == 0:
        rows = [[(buf[i].id, buf[i].score, buf[i].src_in, buf[i].dst_in, buf[i].len)
                 for i in range(int(offs[k]), int(offs[k + 1]))] for k in range(len(hs))]
    return rc, rows, offs


def _single(L, handle, hash_, thresh, skip, src_in, fn="cbh_vidx_find_frame", cap=4096):
    from cbird_amd import _lib

    buf = (_lib.cbh_vmatch * cap)()
    n = C.c_size_t(0)
    _lib.check(getattr(L, fn)(handle, int(hash_), thresh, skip, src_in, buf, cap, C.byref(n)), fn)
    assert n.value <= cap
    return [(buf[i].id, buf[i].score, buf[i].src_in, buf[i].dst_in, buf[i].len) for i in range(n.value)]


# ---- 1. the real RadixMap's committed answers, every needle in one call ------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shards", [None, (1, 3)], ids=["plain", "sharded"])
def test_gpu_find_frames_batch_equals_radixmap_golden(gpu, shards):
    from cbird_amd.video import DctVideoIndex, VideoSearchParams

    g = load_golden("radixmap_r0_r10.npz")
    offs = g["clip_offs"]
    clips = [(g["frames"][a:b], g["hashes"][a:b]) for a, b in zip(offs[:-1], offs[1:])]
    media = _video_media(clips, g["media_ids"].tolist())
    needles = [_M(1, q) for q in g["needles"].tolist()]
    n_rows = 0
    for radix, compat in ((0, True), (0, False), (10, True)):
        idx = DctVideoIndex(radix_compat=compat, shards=shards)
        idx.add(media)
        for thr in g["thresholds"].tolist():
            p = VideoSearchParams(dctThresh=thr, skipFrames=0, minFramesMatched=1, minFramesNear=1, videoRadix=radix)
            got = [_rows(r) for r in idx.find_frames_batch(needles, p)]
            key = f"r{radix}_t{thr}_frame"
            for qi in range(len(needles)):
                a, b = g[key + "_offs"][qi], g[key + "_offs"][qi + 1]
                want = [(int(m), int(d), 0, int(f), 1) for m, d, f in g[key][a:b]]
                assert got[qi] == want, (radix, compat, thr, qi)
                n_rows += len(want)
    assert n_rows > 700


# ---- 2. the batch equals one findFrame per needle and the oracle --------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("skip", [0, 40])
def test_gpu_find_frames_batch_equals_one_by_one(gpu, vorc, skip):
    from cbird_amd import synth_video
    from cbird_amd.video import DctVideoIndex, VideoSearchParams

    clips = synth_video.make_clips(300, 300, seed=11, subclip_frac=0.1, max_gap=8)
    media = _video_media(clips, range(100, 400))
    idx = DctVideoIndex()
    idx.add(media)
    entries = vorc.build_entries([(m.id, f, h) for m, (f, h) in zip(media, clips)], skip)
    assert idx.entries(skip) == len(entries[0])
    rng = np.random.default_rng(7)
    mids = [int(h[len(h) // 2]) for _, h in clips[::3]]
    nothing = 0x5A3C96E1D2B4780E  # (asserted below: no entry within any of the thresholds)
    half = len(mids) // 2
    # a zero hash and a hash that matches nothing: each in the first slot, in the last slot and in between
    orders = ([0] + mids[:half] + [nothing, 0] + mids[half:] + [nothing],
              [nothing] + mids[:half] + [0, nothing] + mids[half:] + [0])
    for thr in (2, 5, 7):
        p = VideoSearchParams(dctThresh=thr, skipFrames=skip, minFramesMatched=1, minFramesNear=1)
        assert vorc.find_frame(entries, nothing, thr, -1) == []
        one = {}  # (hash, src_in) -> findFrame's rows, searched once
        n_hits = 0
        for hashes in orders:
            needles = [_M(1000 + i, q, int(rng.choice([-1, 0, 17]))) for i, q in enumerate(hashes)]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")  # ("needle has no dct hash")
                got = [_rows(r) for r in idx.find_frames_batch(needles, p)]
                for m, rows in zip(needles, got):
                    k = (m.dctHash, m.matchRange.dstIn)
                    if k not in one:
                        one[k] = _rows(idx.findFrame(m, p))
                        want = vorc.find_frame(entries, m.dctHash, thr, m.matchRange.dstIn) if m.dctHash else []
                        assert one[k] == want, (thr, skip, k)
                    assert rows == one[k], (thr, skip, m.id)
                    n_hits += len(rows)
        assert n_hits >= len(mids)
    assert got[0] == [] and got[-1] == [] and got[half + 1] == [] and got[half + 2] == []


# ---- 3. run shapes: the smallest at which the per-run reduction can go wrong --------------------------------------------
def _bit(*bits):
    x = 0
    for b in bits:
        x |= 1 << b
    return x


def _run_shape_videos():
    """-> [(media id, frames, hashes)] in video order, the rows a needle H must get, the rows a needle FAR0 must get.
    Every hash has 5..59 ones, so the insert filter keeps every frame."""
    far = [(~H & (2**64 - 1)) ^ (0xF << (4 * j + 4)) for j in range(5)]  # 64 - 4 bits from H, 8 from each other
    v2 = [H ^ _bit(1 + j % 50) for j in range(300)]
    # entry position 265 of the index: 1 + 70 entries stand before this video.  With H searched alone its run is records
    # 71..370, across the 256-thread block boundary, and the minimum in the wave of records 256..319, an inner one
    v2[265 - 71] = H
    a, b = H ^ _bit(3, 4), H ^ _bit(5, 6)
    videos = [
        (100, [0], [H ^ _bit(10)]),                                  # a one-frame video
        (101, list(range(70)), [H] * 70),                            # 70 identical frames: the run crosses a wave
        (102, [3 * j for j in range(300)], v2),
        (103, [5 * j for j in range(10)], [a, b] * 5),               # two hashes equidistant from H: the earliest wins
        (104, [0, 1, 2], [H ^ _bit(7)] * 3),                         # two videos of one media id: two rows; the last
        (104, [0, 4], [H ^ _bit(8, 9), H]),                          # entry of one and the first of the next both match
        (105, [2 * j for j in range(5)], far),
    ]
    for _, f, h in videos:
        assert len(f) == len(h) and all(5 <= bin(x).count("1") <= 59 for x in h)
    rows_h = [(100, 1, 0), (101, 0, 0), (102, 0, 3 * (265 - 71)), (103, 2, 0), (104, 1, 0), (104, 0, 4)]
    return videos, rows_h, [(105, 0, 0)], far[0]


def _run_shape_needles():
    """H 130 times, mixed with a needle of one record, a needle of none and a zero hash -> hashes, records before each"""
    nothing = H ^ 0xFFFF0000
    _, _, _, far0 = _run_shape_videos()
    hashes = []
    for k in range(130):
        hashes.append(H)
        if k % 2 == 0:
            hashes.append(far0)
        if k % 7 == 3:
            hashes.append(nothing)
        if k % 11 == 5:
            hashes.append(0)
    return hashes, far0, nothing


def test_run_shape_needles_put_the_runs_at_every_alignment():
    """arithmetic on the inputs of the test below: a needle H has 386 records, a needle FAR0 one; the 70-frame run of
    the k-th H begins one record into that needle's records"""
    hashes, far0, _ = _run_shape_needles()
    before, starts = 0, set()
    for q in hashes:
        if q == H:
            starts.add((before + 1) % 64)
            before += 1 + 70 + 300 + 10 + 3 + 2
        elif q == far0:
            before += 1
    assert hashes.count(H) == 130 and len(starts) == 64


@pytest.mark.gpu
@pytest.mark.parametrize("shards", [None, (1, 3)], ids=["plain", "sharded"])
def test_gpu_find_frames_batch_run_shapes(gpu, vorc, shards):
    from cbird_amd import _lib
    from cbird_amd.video import DctVideoIndex, VideoIndex

    videos, rows_h, rows_far, far0 = _run_shape_videos()
    hashes, _, nothing = _run_shape_needles()
    idx = DctVideoIndex(shards=shards)
    for mid, f, h in videos:
        idx._add_one(mid, VideoIndex(f, h))
    n_frames = sum(len(f) for _, f, _ in videos)
    assert idx.entries(0) == n_frames == 391
    entries = vorc.build_entries(videos, 0)
    L = _lib.lib()
    src_in = [(-1, 0, 17)[i % 3] for i in range(len(hashes))]
    rc, got, offs = _raw_batch(L, idx.handle, hashes, src_in, 3, 0, cap=8 * len(hashes))
    assert rc == 0
    for i, (q, s) in enumerate(zip(hashes, src_in)):
        base = rows_h if q == H else rows_far if q == far0 else []
        want = [(m, d, max(s, 0), f, 1) for m, d, f in base]
        assert got[i] == want, i
        if q in (H, far0, nothing) and i < 12:
            assert vorc.find_frame(entries, q, 3, s) == want
    assert int(offs[-1]) == 130 * 6 + hashes.count(far0)
    # H alone: the run of video 102 is records 71..370 of the call, the minimum at record 265
    rc, got, _ = _raw_batch(L, idx.handle, [H], None, 3, 0, cap=16)
    assert rc == 0 and got == [[(m, d, 0, f, 1) for m, d, f in rows_h]]
    assert got[0] == _single(L, idx.handle, H, 3, 0, -1) == vorc.find_frame(entries, H, 3, -1)


# ---- 4. searchIndex ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_search_index_batch_image_and_mixed_needles_equal_per_needle(gpu):
    from cbird_amd import synth_video
    from cbird_amd.database import search_index, search_index_batch
    from cbird_amd.video import DctVideoIndex, VideoSearchParams

    clips = synth_video.make_clips(150, 200, seed=5, subclip_frac=0.2, max_gap=8)
    media = _video_media(clips, range(100, 250))
    idx = DctVideoIndex()
    idx.add(media)
    id_map = {m.id: m for m in media if m.id % 11 != 0}
    # image needles: frames of the videos under the id of their video (filterSelf then has a self to filter), a few
    # bits away so that the lowest thresholds find nothing and the needle escalates
    images = []
    for k, m in enumerate(media[::2]):
        h = m.videoIndex.hashes[len(m.videoIndex.hashes) // 2] ^ _bit(*range(5, 5 + k % 4))
        images.append(_M(m.id, h, (-1, 0, 17)[k % 3]))
    images[3].dctHash = 0
    mixed = [x for pair in zip(images[:40], media[1:80:2]) for x in pair]
    key = lambda g: [(x.id, x.score, x.matchRange.srcIn, x.matchRange.dstIn, x.matchRange.len) for x in g]
    escalated = 0
    for kw in (dict(dctThresh=5, filterSelf=False), dict(dctThresh=1, maxThresh=7, minMatches=1, filterSelf=True),
               dict(dctThresh=2, maxThresh=4, minMatches=2, maxMatches=2, filterSelf=False)):
        p = VideoSearchParams(skipFrames=0, minFramesMatched=10, minFramesNear=30, **kw)
        p.algo = p.AlgoVideo
        for needles in (images, mixed):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                got = search_index_batch(idx, needles, p, id_map)
                want = [search_index(idx, m, p, id_map) for m in needles]
                if p.maxThresh:
                    escalated += sum(len(idx.find(m, p)) <= p.minMatches for m in images[:10])
            assert [key(g) for g in got] == [key(g) for g in want], kw
            assert any(len(g) for g, m in zip(got, needles) if getattr(m, "videoIndex", None) is None)
    assert escalated > 0


# ---- 5. concurrent callers share a batched search -----------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_find_frame_coalesced_equals_find_frame(gpu):
    from cbird_amd import _lib, synth_video
    from cbird_amd.video import DctVideoIndex

    clips = synth_video.make_clips(120, 200, seed=3, subclip_frac=0.15, max_gap=8)
    idx = DctVideoIndex()
    idx.add(_video_media(clips, range(100, 220)))
    L = _lib.lib()
    T, per = 32, 12
    jobs = [[(int(clips[(7 * t + 3 * j) % 120][1][50 + j]), (4, 7)[(t + j) % 2], (-1, 0, 17)[j % 3]) for j in range(per)]
            for t in range(T)]
    jobs[0][0] = (0, 7, -1)  # no dct hash
    want = [[_single(L, idx.handle, q, thr, 0, s) for q, thr, s in job] for job in jobs]
    assert sum(len(r) for w in want for r in w) > T * per // 2
    f0, r0 = C.c_uint64(0), C.c_uint64(0)
    assert L.cbh_combine_stats(idx.handle, C.byref(f0), C.byref(r0)) == 0
    got = [None] * T
    start = threading.Barrier(T)

    def work(t):
        start.wait()
        got[t] = [_single(L, idx.handle, q, thr, 0, s, fn="cbh_vidx_find_frame_coalesced") for q, thr, s in jobs[t]]

    th = [threading.Thread(target=work, args=(t,)) for t in range(T)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert got == want
    f1, r1 = C.c_uint64(0), C.c_uint64(0)
    assert L.cbh_combine_stats(idx.handle, C.byref(f1), C.byref(r1)) == 0
    finds, rounds = f1.value - f0.value, r1.value - r0.value
    assert finds == T * per - 1  # (the needle without a hash is answered before the queue)
    assert 0 < rounds < finds


# ---- 6. edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_find_frames_batch_edges(gpu, vorc):
    from cbird_amd import _lib
    from cbird_amd.video import DctVideoIndex, VideoIndex, VideoSearchParams

    videos, rows_h, _, far0 = _run_shape_videos()
    L = _lib.lib()
    idx = DctVideoIndex()
    for mid, f, h in videos:
        idx._add_one(mid, VideoIndex(f, h))
    offs = np.zeros(4, np.uint64)
    buf = (_lib.cbh_vmatch * 64)()
    q = np.array([H, far0, H], np.uint64)
    assert L.cbh_vidx_find_frames_batch(idx.handle, None, None, 0, 3, 0, buf, 64, offs.ctypes.data) == 0  # n = 0
    assert L.cbh_vidx_find_frames_batch(idx.handle, None, None, 0, 3, 0, None, 0, offs.ctypes.data) == 0
    assert offs[0] == 0
    assert L.cbh_vidx_find_frames_batch(idx.handle, q.ctypes.data, None, 3, 3, 0, buf, 64, None) == _lib.CBH_E_INVAL
    assert L.cbh_vidx_find_frames_batch(idx.handle, q.ctypes.data, None, 3, 3, 0, None, 64, offs.ctypes.data) == _lib.CBH_E_INVAL
    assert L.cbh_vidx_find_frames_batch(idx.handle, None, None, 3, 3, 0, buf, 64, offs.ctypes.data) == _lib.CBH_E_INVAL
    assert L.cbh_vidx_find_frames_batch(None, q.ctypes.data, None, 3, 3, 0, buf, 64, offs.ctypes.data) == _lib.CBH_E_INVAL
    n = C.c_size_t(0)
    assert L.cbh_vidx_find_frame_coalesced(idx.handle, H, 3, 0, -1, None, 4, C.byref(n)) == _lib.CBH_E_INVAL
    assert L.cbh_vidx_find_frame_coalesced(idx.handle, H, 3, 0, -1, buf, 4, None) == _lib.CBH_E_INVAL
    cnt = np.zeros(3, np.uint32)
    ids = np.array([1, 2, 3], np.uint32)
    args = (3, 0, 0, 1, 5, 0, None, 0)
    assert L.cbh_vidx_search_index_frames_batch(idx.handle, None, None, ids.ctypes.data, 3, *args, buf, cnt.ctypes.data) == _lib.CBH_E_INVAL
    assert L.cbh_vidx_search_index_frames_batch(idx.handle, q.ctypes.data, None, ids.ctypes.data, 3, *args, None, cnt.ctypes.data) == _lib.CBH_E_INVAL
    assert L.cbh_vidx_search_index_frames_batch(idx.handle, q.ctypes.data, None, ids.ctypes.data, 3, *args, buf, None) == _lib.CBH_E_INVAL
    assert L.cbh_vidx_search_index_frames_batch(idx.handle, None, None, None, 0, *args, None, None) == 0
    # cap one short: the exact need, and the retry succeeds
    want = [[(m, d, 0, f, 1) for m, d, f in rows_h], [(105, 0, 0, 0, 1)], [(m, d, 0, f, 1) for m, d, f in rows_h]]
    rc, rows, offs = _raw_batch(L, idx.handle, q, None, 3, 0, cap=12)
    assert rc == _lib.CBH_E_OVERFLOW and rows is None and offs.tolist() == [0, 6, 7, 13]
    rc, rows, offs = _raw_batch(L, idx.handle, q, None, 3, 0, cap=13)
    assert rc == 0 and rows == want and offs.tolist() == [0, 6, 7, 13]
    # a threshold <= 0 and an empty index: empty lists
    for thr in (0, -3):
        rc, rows, offs = _raw_batch(L, idx.handle, q, None, thr, 0, cap=13)
        assert rc == 0 and rows == [[], [], []] and offs.tolist() == [0, 0, 0, 0]
    empty = DctVideoIndex()
    rc, rows, offs = _raw_batch(L, empty.handle, q, None, 3, 0, cap=13)
    assert rc == 0 and rows == [[], [], []]
    p = VideoSearchParams(dctThresh=3, skipFrames=0)
    assert empty.find_frames_batch([_M(1, H)], p) == [[]] and empty.find_frames_batch([], p) == []


@pytest.mark.gpu
@pytest.mark.parametrize("shards", [None, (1, 3)], ids=["plain", "sharded"])
def test_gpu_find_frames_batch_survives_every_failed_allocation(gpu, shards):
    """the walk of tests/test_error_paths.py: on a FRESH handle the k-th allocation of the call fails once, k = 0, 1, ..
    until the call makes fewer; the call absorbs it or returns CBH_E_NOMEM (CBH_E_OVERFLOW where a record block could
    not grow), and the next clean call on the same handle gives the right answer"""
    from cbird_amd import _lib
    from cbird_amd.video import DctVideoIndex, VideoIndex

    videos, rows_h, _, far0 = _run_shape_videos()
    L = _lib.lib()
    q = [H, far0, 0, H]
    want = [[(m, d, 0, f, 1) for m, d, f in rows_h], [(105, 0, 0, 0, 1)], [], [(m, d, 0, f, 1) for m, d, f in rows_h]]

    def tuning(key):
        v = C.c_longlong(-2)
        assert L.cbh_get_tuning(key, C.byref(v)) == 0
        return int(v.value)

    failed = 0
    for k in range(200):
        idx = DctVideoIndex(shards=shards)
        for mid, f, h in videos:
            idx._add_one(mid, VideoIndex(f, h))
        fired0 = tuning(b"fault_fired")
        L.cbh_set_tuning(b"fault_alloc_after", k)
        try:
            rc, rows, _ = _raw_batch(L, idx.handle, q, None, 3, 0, cap=64)
        finally:
            L.cbh_set_tuning(b"fault_alloc_after", -1)
        if tuning(b"fault_fired") == fired0:
            assert rc == 0 and rows == want
            break
        failed += 1
        assert (rc == 0 and rows == want) or rc in (_lib.CBH_E_NOMEM, _lib.CBH_E_OVERFLOW, _lib.CBH_E_NODEVICE), (k, rc)
        rc, rows, _ = _raw_batch(L, idx.handle, q, None, 3, 0, cap=64)
        assert rc == 0 and rows == want, k
    else:
        pytest.fail("the call never ran out of allocations to fail")
    assert failed >= 8  # the build's arrays, evidx, the workspace, and the reduction's seven scratch blocks at the least
