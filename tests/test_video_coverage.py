"""GPU: cbh_video_coverage / cbh_vidx_coverage (cbird_amd/csrc/vcoverage.hip) equal the NumPy model of
tests/video_coverage_rules.py bit for bit -- the hand vectors, every wave / tile / chunk edge at forced-small and at
default knobs, a ragged batch over shared videos, the capacity protocol, plain and sharded handles, error codes, refused
allocations -- and agree with cbh_vidx_find_videos_batch, which this feature does not touch."""
import ctypes as C

import numpy as np
import pytest

import video_coverage_rules as VR
from cbird_amd.video import VCOVER_DTYPE, VCOVER_FRAME_DTYPE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(gpu):
    from cbird_amd import _lib

    return _lib.lib()


def _tuning(L, key):
    v = C.c_longlong(0)
    assert L.cbh_get_tuning(key, C.byref(v)) == 0
    return v.value


@pytest.fixture
def knobs(lib):
    """sets "vcover_chunk" / "vcover_tile" for one test and puts the defaults back"""
    def set_(chunk=0, tile=1024):
        assert lib.cbh_set_tuning(b"vcover_chunk", chunk) == 0 and lib.cbh_set_tuning(b"vcover_tile", tile) == 0
    yield set_
    set_()


def table(videos):
    f = np.concatenate([np.asarray(v[0], np.int32) for v in videos] + [np.zeros(0, np.int32)])
    h = np.concatenate([np.asarray(v[1], np.uint64) for v in videos] + [np.zeros(0, np.uint64)])
    o = np.zeros(len(videos) + 1, np.uint64)
    np.cumsum([len(v[0]) for v in videos], out=o[1:])
    return f, h, o


def cover(L, videos, pairs, thresh, skip, maps=True, cap=None):
    """(rc, summaries, map, offsets) of one cbh_video_coverage call; with maps the two calls of the capacity protocol"""
    f, h, o = table(videos)
    p = np.ascontiguousarray(np.asarray(pairs, np.uint32).reshape(-1, 2))
    sums = np.zeros(max(1, len(p)), VCOVER_DTYPE)
    offs = np.zeros(len(p) + 1, np.uint64)

    def call(m, cap):
        return L.cbh_video_coverage(0, f.ctypes.data, h.ctypes.data, o.ctypes.data, len(videos), p.ctypes.data, len(p), thresh,
                                    skip, sums.ctypes.data, None if m is None else m.ctypes.data, cap, offs.ctypes.data)

    if not maps:
        return call(None, 0), sums[:len(p)], None, offs
    if cap is None:
        from cbird_amd import _lib
        one = np.zeros(1, VCOVER_FRAME_DTYPE)
        assert call(one, 0) == (_lib.CBH_E_OVERFLOW if int(offs[-1]) else 0)
        cap = int(offs[-1])
    m = np.zeros(max(1, cap), VCOVER_FRAME_DTYPE)
    return call(m, cap), sums[:len(p)], m[:int(offs[-1])], offs


_model_cache = {}


def model(videos, pairs, thresh, skip, key=None):
    """what the call must return: summaries, the concatenated map and its offsets"""
    sums = np.zeros(len(pairs), VCOVER_DTYPE)
    maps, offs = [], [0]
    for k, (a, b) in enumerate(pairs):
        ck = (key, a, b, thresh, skip)
        if key is None or ck not in _model_cache:
            _model_cache[ck] = VR.coverage(videos[a], videos[b], thresh, skip)
        s, frames, dframes, dist = _model_cache[ck]
        for name in VR.FIELDS:
            sums[k][name] = s[name]
        m = np.zeros(len(frames), VCOVER_FRAME_DTYPE)
        m["src_frame"], m["dst_frame"], m["distance"] = frames, dframes, dist
        maps.append(m)
        offs.append(offs[-1] + len(frames))
    return sums, np.concatenate(maps + [np.zeros(0, VCOVER_FRAME_DTYPE)]), np.array(offs, np.uint64)


def same(got, want):
    rc, sums, m, offs = got
    assert rc == 0
    assert offs.tolist() == want[2].tolist()
    for name in VCOVER_DTYPE.names:
        assert sums[name].tolist() == want[0][name].tolist(), name
    if m is not None:
        assert m.tobytes() == want[1].tobytes()


@pytest.mark.parametrize("name", list(VR.HAND))
def test_hand_vectors(lib, name):
    src, dst, thresh, skip, want = VR.HAND[name]
    got = cover(lib, [src, dst], [(0, 1)], thresh, skip)
    same(got, model([src, dst], [(0, 1)], thresh, skip))
    for key, value in want.items():  # and what was written down by hand, without the model in between
        column = {"frames": "src_frame", "dst_frames": "dst_frame", "distances": "distance"}.get(key)
        assert (got[2][column].tolist() if column else int(got[1][0][key])) == value, key


# ---- sizes: every wave, tile, stage and chunk edge ------------------------------------------------------------------------
SRC_LENGTHS = [1, 63, 64, 65, 255, 256, 257, 1025]  # 1025: one above the default tile; 257: one above a tile of 256
DST_LENGTHS = [0, 1, 63, 64, 65, 129, 255, 256, 257, 600]  # around a chunk of 64 and around the 256-entry LDS stage


@pytest.fixture(scope="module")
def sized():
    """sources and destinations cut from one random walk (2 bit flips a frame: near frames, many equal distances), the
    destinations with a bit of noise and a few low-detail hashes; every source against every destination"""
    rng = np.random.default_rng(5)
    n = 1100
    step = np.zeros(n, np.uint64)
    for _ in range(2):
        step ^= np.uint64(1) << rng.integers(0, 64, n).astype(np.uint64)
    step[0] = rng.integers(0, 2**63, dtype=np.uint64)
    walk = np.bitwise_xor.accumulate(step)
    frames = np.cumsum(rng.integers(1, 6, n)).astype(np.int32) - 1
    videos = [(frames[:m] - frames[0], walk[:m].copy()) for m in SRC_LENGTHS]
    for m in DST_LENGTHS:
        a = int(rng.integers(0, n - m + 1))
        h = walk[a:a + m] ^ np.where(rng.random(m) < 0.3, np.uint64(1) << rng.integers(0, 64, m).astype(np.uint64), np.uint64(0))
        h[rng.random(m) < 0.02] = np.uint64(7)  # no entries
        videos.append(((frames[a:a + m] - (frames[a] if m else 0)).astype(np.int32), h))
    pairs = [(a, len(SRC_LENGTHS) + b) for a in range(len(SRC_LENGTHS)) for b in range(len(DST_LENGTHS))]
    return videos, pairs, model(videos, pairs, 5, 0)


@pytest.mark.parametrize("chunk,tile", [(64, 1024), (64, 256), (1, 512), (0, 1024), (0, 2048), (100, 256)])
def test_sizes_at_forced_and_default_knobs(lib, knobs, sized, chunk, tile):
    """a chunk of 64 makes up to ten chunks of one pair meet by atomicMin; (0, 1024) are the defaults: the same bytes"""
    videos, pairs, want = sized
    knobs(chunk, tile)
    assert (_tuning(lib, b"vcover_chunk"), _tuning(lib, b"vcover_tile")) == (chunk, tile)
    same(cover(lib, videos, pairs, 5, 0), want)


def test_knobs_refuse_what_they_cannot_take(lib, knobs):
    for key, bad in ((b"vcover_chunk", -1), (b"vcover_chunk", (1 << 24) + 1), (b"vcover_tile", 0), (b"vcover_tile", 300)):
        before = _tuning(lib, key)
        assert lib.cbh_set_tuning(key, bad) == -1 and _tuning(lib, key) == before


def test_trim_on_long_videos(lib, knobs, sized):
    """skip on: sources lose both ends, destinations only when long enough; chunked and not"""
    videos, pairs, _ = sized
    pairs = [p for p in pairs if p[0] >= 4]
    want = model(videos, pairs, 7, 40)
    assert len(set(want[0]["n_src"].tolist())) > 2 and 0 in want[0]["n_dst"].tolist()
    same(cover(lib, videos, pairs, 7, 40), want)
    knobs(64, 256)
    same(cover(lib, videos, pairs, 7, 40), want)


# ---- the 12 clips: a ragged batch over shared videos ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def clips():
    return VR.clips()


ALL_PAIRS = [(a, b) for a in range(12) for b in range(12)]  # 144: src == dst and both directions of every pair


@pytest.mark.parametrize("skip", [0, 20])
def test_ragged_batch_over_shared_videos(lib, knobs, clips, skip):
    want = model(clips, ALL_PAIRS, 5, skip, key="clips")
    same(cover(lib, clips, ALL_PAIRS, 5, skip), want)
    knobs(16, 256)
    same(cover(lib, clips, ALL_PAIRS, 5, skip), want)
    # a video may be named by one pair only, and a pair may be named twice
    some = [(11, 2), (2, 11), (5, 5), (11, 2)]
    same(cover(lib, clips, some, 5, skip), model(clips, some, 5, skip, key="clips"))


def test_summaries_only_and_the_capacity_protocol(lib, clips):
    from cbird_amd import _lib

    want = model(clips, ALL_PAIRS, 5, 0, key="clips")
    rc, sums, m, offs = cover(lib, clips, ALL_PAIRS, 5, 0, maps=False)
    same((rc, sums, m, offs), want)  # (the offsets are filled without a map too)
    need = int(want[2][-1])
    # too little room: CBH_E_OVERFLOW, the offsets complete, the needed capacity in the last, nothing else written
    rc, sums, m, offs = cover(lib, clips, ALL_PAIRS, 5, 0, cap=need - 1)
    assert rc == _lib.CBH_E_OVERFLOW and offs.tolist() == want[2].tolist() and int(offs[-1]) == need
    assert not sums.tobytes().strip(b"\0") and not m.tobytes().strip(b"\0")
    same(cover(lib, clips, ALL_PAIRS, 5, 0, cap=need), want)
    same(cover(lib, clips, ALL_PAIRS, 5, 0), want)  # cap 0 first, then what it asked for


def handle_of(gpu, clips, shards=None):
    from cbird_amd.video import DctVideoIndex, VideoIndex
    from cbird_amd import Media

    index = DctVideoIndex(shards=shards)
    media = []
    for i, (f, h) in enumerate(clips):
        m = Media(id=i + 1, path=f"{i + 1}.mp4")
        m.videoIndex = VideoIndex(f.tolist(), [int(x) for x in h])
        media.append(m)
    index.add(media)
    return index, media


def vidx_cover(L, index, pairs, thresh, skip, maps=True):
    s = np.ascontiguousarray([a + 1 for a, _ in pairs], np.uint32)
    d = np.ascontiguousarray([b + 1 for _, b in pairs], np.uint32)
    sums = np.zeros(max(1, len(pairs)), VCOVER_DTYPE)
    offs = np.zeros(len(pairs) + 1, np.uint64)
    one = np.zeros(1, VCOVER_FRAME_DTYPE)
    rc = L.cbh_vidx_coverage(index.handle, s.ctypes.data, d.ctypes.data, len(pairs), thresh, skip, sums.ctypes.data,
                             one.ctypes.data if maps else None, 0, offs.ctypes.data)
    if not maps or rc != -6:
        return rc, sums[:len(pairs)], None, offs
    m = np.zeros(int(offs[-1]), VCOVER_FRAME_DTYPE)
    rc = L.cbh_vidx_coverage(index.handle, s.ctypes.data, d.ctypes.data, len(pairs), thresh, skip, sums.ctypes.data,
                             m.ctypes.data, len(m), offs.ctypes.data)
    return rc, sums[:len(pairs)], m, offs


@pytest.mark.parametrize("skip", [0, 20])
def test_agrees_with_find_videos_batch(gpu, lib, clips, skip):
    """code this feature does not touch: every match of cbh_vidx_find_videos_batch (no self filter, one frame enough, any
    locality) is (100 - near_percent, src_in, dst_in, len) of its pair, and a pair has no match exactly when nothing of it
    is covered.  A fresh handle per skip: a built search structure keeps its first skip."""
    from cbird_amd.video import VideoSearchParams

    index, media = handle_of(gpu, clips)
    p = VideoSearchParams(dctThresh=5, skipFrames=skip, minFramesMatched=1, minFramesNear=0, filterSelf=False)
    found = index.find_videos_batch(media, p)
    rc, sums, _, _ = vidx_cover(lib, index, ALL_PAIRS, 5, skip, maps=False)
    assert rc == 0
    matches = 0
    for a in range(12):
        by_id = {m.mediaId: m for m in found[a]}
        assert len(by_id) == len(found[a])
        for b in range(12):
            s = sums[a * 12 + b]
            if int(s["n_covered"]) == 0:
                assert b + 1 not in by_id, (a, b)
                continue
            m = by_id[b + 1]
            assert (m.score, m.range.srcIn, m.range.dstIn, m.range.len) == \
                (100 - int(s["near_percent"]), int(s["src_in"]), int(s["dst_in"]), int(s["len"])), (a, b)
            matches += 1
    assert matches == sum(len(f) for f in found) >= 12 + 8


@pytest.mark.parametrize("skip", [0, 20])
def test_plain_and_sharded_handles(gpu, lib, clips, skip):
    want = model(clips, ALL_PAIRS, 5, skip, key="clips")
    plain, _ = handle_of(gpu, clips)
    sharded, _ = handle_of(gpu, clips, shards=(1, 5))
    same(vidx_cover(lib, plain, ALL_PAIRS, 5, skip), want)
    same(vidx_cover(lib, sharded, ALL_PAIRS, 5, skip), want)
    assert sharded.entries(skip) == plain.entries(skip)  # a built structure changes nothing
    same(vidx_cover(lib, sharded, ALL_PAIRS[:50], 5, skip), model(clips, ALL_PAIRS[:50], 5, skip, key="clips"))


def test_a_doubled_id_means_its_first_video(gpu, lib, clips):
    index, _ = handle_of(gpu, clips[:3])
    f, h = clips[5]
    assert lib.cbh_vidx_add_video(index.handle, 2, f.ctypes.data, h.ctypes.data, len(f)) == 0  # a second video of id 2
    same(vidx_cover(lib, index, [(1, 0), (0, 1), (1, 1)], 5, 0), model(clips, [(1, 0), (0, 1), (1, 1)], 5, 0, key="clips"))


def test_python_entry_points(gpu, clips):
    from cbird_amd.database import video_coverage
    from cbird_amd.index import SearchParams
    from cbird_amd.video import VideoSearchParams, video_coverage as coverage_of_lists

    index, media = handle_of(gpu, clips)
    p = VideoSearchParams(algo=SearchParams.AlgoVideo, dctThresh=5, skipFrames=0)
    pairs = [(9, 7), (7, 9), (4, 4), (1, 12)]
    for got in (index.coverage(pairs, p), coverage_of_lists(clips, [(a - 1, b - 1) for a, b in pairs], 5, 0)):
        for c, (a, b) in zip(got, pairs):
            s, frames, dframes, dist = VR.coverage(clips[a - 1], clips[b - 1], 5, 0)
            assert {k: getattr(c, k) for k in VR.FIELDS} == s
            assert (c.frames.tolist(), c.dst_frames.tolist(), c.distances.tolist()) == \
                (frames.tolist(), dframes.tolist(), dist.tolist())
            spans = VR.source_view(*clips[a - 1], 0)[1]
            assert c.ranges() == VR.ranges(frames, spans, dist < 5) and c.ranges(False) == VR.ranges(frames, spans, dist >= 5)
    assert got[0].contains() and not got[1].contains() and got[2].contains() and got[2].ranges(False) == []
    bare = index.coverage(pairs, p, maps=False)
    assert [b.frames for b in bare] == [None] * 4 and [b.percent() for b in bare] == [c.percent() for c in got]
    assert index.coverage([], p) == []
    groups = [[media[8], media[6]], [media[6], media[8]]]
    video_coverage(index, groups, p)
    assert (groups[0][1].coverage, groups[1][1].coveredBy) == (100, 100)
    assert groups[0][1].coveredBy == groups[1][1].coverage == got[1].percent() < 100


def test_error_codes(gpu, lib, clips):
    from cbird_amd import _lib

    f, h, o = table(clips[:2])
    p = np.array([[0, 1]], np.uint32)
    sums = np.full(1, -1, np.int64).repeat(9).view(VCOVER_DTYPE)
    offs = np.full(3, 77, np.uint64)
    m = np.zeros(100, VCOVER_FRAME_DTYPE)

    def call(frames=f.ctypes.data, hashes=h.ctypes.data, voff=o.ctypes.data, n_videos=2, pairs=p.ctypes.data, n_pairs=1,
             skip=0, s=sums.ctypes.data, map_=m.ctypes.data, cap=100, offsets=offs.ctypes.data, device=0):
        return lib.cbh_video_coverage(device, frames, hashes, voff, n_videos, pairs, n_pairs, 5, skip, s, map_, cap, offsets)

    for bad in (dict(frames=None), dict(hashes=None), dict(voff=None), dict(pairs=None), dict(s=None), dict(offsets=None),
                dict(skip=-1), dict(n_videos=1)):
        assert call(**bad) == _lib.CBH_E_INVAL, bad
        assert lib.cbh_last_error()  # (a text says which)
    assert call(device=99) == _lib.CBH_E_NODEVICE
    assert sums.tobytes() == np.full(9, -1, np.int64).tobytes() and offs.tolist() == [77, 77, 77]  # nothing was written
    assert call(n_pairs=0) == 0 and offs.tolist() == [0, 77, 77]
    assert call(n_pairs=0, pairs=None, s=None, map_=None, offsets=None, frames=None, hashes=None) == 0
    assert call(map_=None, offsets=None) == 0 and int(sums[0]["n_src"]) == len(clips[0][0])
    falling = np.array([0, 70, 60], np.uint64)
    assert call(voff=falling.ctypes.data) == _lib.CBH_E_INVAL

    index, _ = handle_of(gpu, clips[:3])
    ids = np.array([1, 2], np.uint32)
    unknown = np.array([2, 9], np.uint32)
    sums[:] = np.full(9, -1, np.int64).view(VCOVER_DTYPE)
    offs[:] = 77

    def vcall(handle=index.handle, src=ids.ctypes.data, dst=ids.ctypes.data, n=2, s=None):
        big = np.zeros(2, VCOVER_DTYPE)
        return lib.cbh_vidx_coverage(handle, src, dst, n, 5, 0, s if s is not None else big.ctypes.data, None, 0, offs.ctypes.data)

    assert vcall(dst=unknown.ctypes.data, s=sums.ctypes.data) == _lib.CBH_E_INVAL  # an id the handle does not hold
    assert sums.tobytes() == np.full(9, -1, np.int64).tobytes() and offs.tolist() == [77, 77, 77]
    assert vcall(handle=None) == _lib.CBH_E_INVAL and vcall(src=None) == _lib.CBH_E_INVAL
    assert vcall(n=0, src=None, dst=None) == 0
    assert vcall() == 0 and offs.tolist() == [0, 70, 70 + len(clips[1][0])]


def test_every_allocation_may_be_refused(gpu, lib, clips):
    """the walk of tests/test_error_paths.py: every refused call returns CBH_E_NOMEM, leaves no scratch handed out and no
    device memory behind, and the handle gives the same answer afterwards"""
    from cbird_amd import _lib

    index, _ = handle_of(gpu, clips)
    pairs = ALL_PAIRS[:30]
    want = model(clips, pairs, 5, 0, key="clips")
    same(vidx_cover(lib, index, pairs, 5, 0), want)
    s = np.ascontiguousarray([a + 1 for a, _ in pairs], np.uint32)
    d = np.ascontiguousarray([b + 1 for _, b in pairs], np.uint32)
    sums, offs = np.zeros(len(pairs), VCOVER_DTYPE), np.zeros(len(pairs) + 1, np.uint64)
    m = np.zeros(int(want[2][-1]), VCOVER_FRAME_DTYPE)

    def run():
        return lib.cbh_vidx_coverage(index.handle, s.ctypes.data, d.ctypes.data, len(pairs), 5, 0, sums.ctypes.data,
                                     m.ctypes.data, len(m), offs.ctypes.data)

    refused = 0
    for k in range(100):
        live0, fired0 = _tuning(lib, b"arena_live_bytes"), _tuning(lib, b"fault_fired")
        lib.cbh_set_tuning(b"fault_alloc_after", k)
        try:
            rc = run()
        finally:
            lib.cbh_set_tuning(b"fault_alloc_after", -1)
        if _tuning(lib, b"fault_fired") == fired0:
            assert rc == 0
            break
        refused += 1
        assert rc == _lib.CBH_E_NOMEM, (k, rc)
        assert _tuning(lib, b"arena_live_bytes") == live0, k
        assert run() == 0 and (sums.tobytes(), m.tobytes()) == (want[0].tobytes(), want[1].tobytes()), k
    else:
        pytest.fail("the call never ran out of allocations to refuse")
    assert refused == 6  # source views, destination views, tables, keys, summaries, map
    assert index.entries(0) > 0
