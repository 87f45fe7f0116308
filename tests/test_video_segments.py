"""GPU: cbh_video_segments / cbh_vidx_segments (cbird_amd/csrc/vsegments.hip) and the Python entries equal the NumPy model
of tests/video_segments_rules.py record for record -- summaries, segments and maps: the hand vectors, the 12-clip set as
one ragged batch over shared videos, every wave and LDS-stage edge, a long static run, the call without maps, the
capacity protocol, the error codes, plain and sharded handles, two settings of "vseg_budget_mb"."""
import ctypes as C

import numpy as np
import pytest

import video_coverage_rules as VR
import video_segments_rules as SR
from cbird_amd.video import VSEGMENT_DTYPE, VSEGMENT_FRAME_DTYPE, VSEGMENTS_DTYPE

pytestmark = pytest.mark.gpu

PAR = dict(thresh=5, skip=0, tol=15, min_frames=3, max_segments=4)


@pytest.fixture(scope="module")
def lib(gpu):
    from cbird_amd import _lib

    return _lib.lib()


def _tuning(L, key):
    v = C.c_longlong(0)
    assert L.cbh_get_tuning(key, C.byref(v)) == 0
    return v.value


@pytest.fixture
def budget(lib):
    """sets "vseg_budget_mb" for one test and puts the default back"""
    def set_(mb=256):
        assert lib.cbh_set_tuning(b"vseg_budget_mb", mb) == 0
    yield set_
    set_()


def table(videos):
    f = np.concatenate([np.asarray(v[0], np.int32) for v in videos] + [np.zeros(0, np.int32)])
    h = np.concatenate([np.asarray(v[1], np.uint64) for v in videos] + [np.zeros(0, np.uint64)])
    o = np.zeros(len(videos) + 1, np.uint64)
    np.cumsum([len(v[0]) for v in videos], out=o[1:])
    return f, h, o


def find(L, videos, pairs, par, maps=True, cap=None):
    """(rc, summaries, segments, map, offsets) of one cbh_video_segments call; with maps the two calls of the protocol"""
    f, h, o = table(videos)
    p = np.ascontiguousarray(np.asarray(pairs, np.uint32).reshape(-1, 2))
    sums = np.zeros(max(1, len(p)), VSEGMENTS_DTYPE)
    segs = np.full(max(1, len(p) * par["max_segments"]), -1, np.int64).repeat(4).view(VSEGMENT_DTYPE)  # (must be zeroed)
    offs = np.zeros(len(p) + 1, np.uint64)

    def call(m, cap):
        return L.cbh_video_segments(0, f.ctypes.data, h.ctypes.data, o.ctypes.data, len(videos), p.ctypes.data, len(p),
                                    par["thresh"], par["skip"], par["tol"], par["min_frames"], par["max_segments"],
                                    sums.ctypes.data, segs.ctypes.data, None if m is None else m.ctypes.data, cap,
                                    offs.ctypes.data)

    if not maps:
        return call(None, 0), sums[:len(p)], segs, None, offs
    if cap is None:
        from cbird_amd import _lib
        one = np.zeros(1, VSEGMENT_FRAME_DTYPE)
        assert call(one, 0) == (_lib.CBH_E_OVERFLOW if int(offs[-1]) else 0)
        cap = int(offs[-1])
    m = np.zeros(max(1, cap), VSEGMENT_FRAME_DTYPE)
    return call(m, cap), sums[:len(p)], segs, m[:int(offs[-1])], offs


_model_cache = {}


def model(videos, pairs, par, key=None):
    """what the call must return: summaries, segment records (unused ones zero), the concatenated map and its offsets"""
    sums = np.zeros(len(pairs), VSEGMENTS_DTYPE)
    segs = np.zeros(max(1, len(pairs) * par["max_segments"]), VSEGMENT_DTYPE)
    maps, offs = [], [0]
    for k, (a, b) in enumerate(pairs):
        ck = (key, a, b) + tuple(sorted(par.items()))
        if key is None or ck not in _model_cache:
            _model_cache[ck] = SR.run(videos[a], videos[b], par)
        s, found, frames, dframes, dist, seg = _model_cache[ck]
        for name in SR.SUMMARY_FIELDS:
            sums[k][name] = s[name]
        for r, g in enumerate(found):
            for name in SR.SEGMENT_FIELDS:
                segs[k * par["max_segments"] + r][name] = g[name]
        m = np.zeros(len(frames), VSEGMENT_FRAME_DTYPE)
        m["src_frame"], m["dst_frame"], m["distance"], m["segment"] = frames, dframes, dist, seg
        maps.append(m)
        offs.append(offs[-1] + len(frames))
    return sums, segs, np.concatenate(maps + [np.zeros(0, VSEGMENT_FRAME_DTYPE)]), np.array(offs, np.uint64)


def same(got, want):
    rc, sums, segs, m, offs = got
    assert rc == 0
    assert offs.tolist() == want[3].tolist()
    for name in VSEGMENTS_DTYPE.names:
        assert sums[name].tolist() == want[0][name].tolist(), name
    for name in VSEGMENT_DTYPE.names:
        assert segs[name].tolist() == want[1][name].tolist(), name
    if m is not None:
        for name in VSEGMENT_FRAME_DTYPE.names:
            assert m[name].tolist() == want[2][name].tolist(), name


@pytest.mark.parametrize("name", list(SR.HAND))
def test_hand_vectors(lib, name):
    src, dst, par, want, segs, columns = SR.hand(name)
    got = find(lib, [src, dst], [(0, 1)], par)
    same(got, model([src, dst], [(0, 1)], par))
    for key, value in want.items():  # and what was written down by hand, without the model in between
        assert int(got[1][0][key]) == value, key
    assert [{n: int(g[n]) for n in SR.SEGMENT_FIELDS} for g in got[2][:len(segs)]] == segs
    for key, value in columns.items():
        column = {"frames": "src_frame", "dst_frames": "dst_frame", "distances": "distance", "segments": "segment"}[key]
        assert got[3][column].tolist() == value, key


def test_all_hand_vectors_in_one_batch_at_one_setting(lib):
    """the hand-made videos as one table: pairs of very different offset domains side by side"""
    names = [n for n in SR.HAND if SR.hand(n)[2] == {**SR.DEFAULTS, "tol": 2}]
    videos, pairs = [], []
    for n in names:
        src, dst, *_ = SR.hand(n)
        pairs.append((len(videos), len(videos) + 1))
        videos += [src, dst]
    par = {**SR.DEFAULTS, "tol": 2}
    assert len(names) >= 10
    same(find(lib, videos, pairs, par), model(videos, pairs, par))


# ---- the 12 clips: a ragged batch over shared videos ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def clips():
    return VR.clips()


ALL_PAIRS = [(a, b) for a in range(12) for b in range(12)]  # 144: src == dst and both directions of every pair


@pytest.mark.parametrize("skip", [0, 20])
def test_ragged_batch_over_shared_videos(lib, budget, clips, skip):
    par = {**PAR, "skip": skip}
    want = model(clips, ALL_PAIRS, par, key="clips")
    assert 12 + 8 <= int((want[0]["n_segments"] > 0).sum()) < 144
    same(find(lib, clips, ALL_PAIRS, par), want)
    # a video may be named by one pair only, a pair may be named twice, a video may meet itself
    some = [(11, 2), (2, 11), (5, 5), (11, 2), (2, 0), (2, 1), (2, 3), (2, 4)]
    same(find(lib, clips, some, par), model(clips, some, par, key="clips"))


@pytest.mark.parametrize("par", [dict(tol=0), dict(tol=3, min_frames=1, max_segments=16), dict(max_segments=1),
                                 dict(thresh=9, min_frames=1, max_segments=2), dict(tol=200, min_frames=30)])
def test_other_parameters_on_the_clips(lib, clips, par):
    par = {**PAR, **par}
    pairs = [(a, b) for a in (1, 6, 8, 9) for b in (1, 6, 8, 9)]
    same(find(lib, clips, pairs, par), model(clips, pairs, par, key="clips"))


# ---- sizes: every wave and stage edge -------------------------------------------------------------------------------------
def test_sizes_around_the_wave_the_tile_and_the_lds_stage(lib):
    """sources of 1, 63, 64, 65, 129 frames against destinations of 1, 255, 256, 257 and 600 entries (the stage holds 256)"""
    videos, pairs = SR.sized_videos()
    par = {**PAR, "min_frames": 1}
    want = model(videos, pairs, par)
    assert int((want[0]["n_segments"] > 0).sum()) >= 10
    same(find(lib, videos, pairs, par), want)


def test_a_source_above_one_tile_and_a_long_difference_array(lib):
    """700 source frames are three tiles of 256; frame numbers up to 60 000 make a difference array of 120 000 words,
    many steps of the prefix pass, with the plateau far from the array's start"""
    rng = np.random.default_rng(13)
    n = 700
    h = rng.integers(0, 2**63, n, dtype=np.uint64)
    f = np.sort(rng.choice(60000, n, replace=False)).astype(np.int32)
    sub = ((f[300:] - f[300]).astype(np.int32), h[300:].copy())
    videos, pairs = [(f, h), sub], [(0, 1), (1, 0), (0, 0)]
    want = model(videos, pairs, PAR)
    assert want[1]["offset"][[0, 4, 8]].tolist() == [-int(f[300]), int(f[300]), 0] and want[1]["n_frames"][8] == 700
    same(find(lib, videos, pairs, PAR), want)


def test_static_run_on_both_sides(lib):
    """300 equal frames on both sides: every one of them matches 300 entries, one long merged interval per lane"""
    videos, pairs = SR.static_videos()
    par = {**PAR, "tol": 2}
    want = model(videos, pairs, par)
    assert want[0]["n_aligned"].min() >= 300
    same(find(lib, videos, pairs, par), want)
    same(find(lib, videos, pairs, PAR), model(videos, pairs, PAR))


# ---- maps, capacity, knobs ------------------------------------------------------------------------------------------------
def test_no_maps_and_the_capacity_protocol(lib, clips):
    from cbird_amd import _lib

    want = model(clips, ALL_PAIRS, PAR, key="clips")
    same(find(lib, clips, ALL_PAIRS, PAR, maps=False), want)  # (the offsets are filled without a map too)
    need = int(want[3][-1])
    # too little room: CBH_E_OVERFLOW, the offsets complete, the needed capacity in the last, nothing else written
    rc, sums, segs, m, offs = find(lib, clips, ALL_PAIRS, PAR, cap=need - 1)
    assert rc == _lib.CBH_E_OVERFLOW and offs.tolist() == want[3].tolist() and int(offs[-1]) == need
    assert not sums.tobytes().strip(b"\0") and not m.tobytes().strip(b"\0") and not segs.tobytes().strip(b"\xff")
    same(find(lib, clips, ALL_PAIRS, PAR, cap=need), want)


def test_budget_knob_changes_groups_not_results(lib, budget):
    """frame numbers up to 200 000 give arrays of 1.6 MB: at 2 MB every pair is a group of its own, at 256 MB all are one"""
    rng = np.random.default_rng(14)
    n = 120
    h = rng.integers(0, 2**63, n, dtype=np.uint64)
    f = np.sort(rng.choice(200000, n, replace=False)).astype(np.int32)
    videos = [(f, h), ((f[30:90] - f[30]).astype(np.int32), h[30:90].copy()), ((f[50:] - f[50]).astype(np.int32), h[50:].copy())]
    pairs = [(a, b) for a in range(3) for b in range(3)]
    want = model(videos, pairs, PAR)
    assert int((want[0]["n_segments"] > 0).sum()) == 9
    for mb in (2, 256):
        budget(mb)
        assert _tuning(lib, b"vseg_budget_mb") == mb
        same(find(lib, videos, pairs, PAR), want)
    from cbird_amd import _lib
    budget(1)  # one array alone is above it: refused, nothing kept
    live = _tuning(lib, b"arena_live_bytes")
    assert find(lib, videos, pairs, PAR, maps=False)[0] == _lib.CBH_E_NOMEM and lib.cbh_last_error()
    assert _tuning(lib, b"arena_live_bytes") == live
    for bad in (0, -1, 4097):
        assert lib.cbh_set_tuning(b"vseg_budget_mb", bad) == -1 and _tuning(lib, b"vseg_budget_mb") == 1


# ---- handles and the Python entries ---------------------------------------------------------------------------------------
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


def vidx_find(L, index, pairs, par, maps=True):
    s = np.ascontiguousarray([a + 1 for a, _ in pairs], np.uint32)
    d = np.ascontiguousarray([b + 1 for _, b in pairs], np.uint32)
    sums = np.zeros(max(1, len(pairs)), VSEGMENTS_DTYPE)
    segs = np.zeros(max(1, len(pairs) * par["max_segments"]), VSEGMENT_DTYPE)
    offs = np.zeros(len(pairs) + 1, np.uint64)
    one = np.zeros(1, VSEGMENT_FRAME_DTYPE)

    def call(m, cap):
        return L.cbh_vidx_segments(index.handle, s.ctypes.data, d.ctypes.data, len(pairs), par["thresh"], par["skip"],
                                   par["tol"], par["min_frames"], par["max_segments"], sums.ctypes.data, segs.ctypes.data, m,
                                   cap, offs.ctypes.data)

    rc = call(one.ctypes.data if maps else None, 0)
    if not maps or rc != -6:
        return rc, sums[:len(pairs)], segs, None, offs
    m = np.zeros(int(offs[-1]), VSEGMENT_FRAME_DTYPE)
    return call(m.ctypes.data, len(m)), sums[:len(pairs)], segs, m, offs


@pytest.mark.parametrize("skip", [0, 20])
def test_plain_and_sharded_handles(gpu, lib, clips, skip):
    par = {**PAR, "skip": skip}
    want = model(clips, ALL_PAIRS, par, key="clips")
    plain, _ = handle_of(gpu, clips)
    sharded, _ = handle_of(gpu, clips, shards=(1, 5))
    same(vidx_find(lib, plain, ALL_PAIRS, par), want)
    same(vidx_find(lib, sharded, ALL_PAIRS, par), want)
    same(vidx_find(lib, sharded, ALL_PAIRS[:50], par, maps=False), model(clips, ALL_PAIRS[:50], par, key="clips"))


def test_python_entry_points(gpu, clips):
    from cbird_amd.database import video_segments
    from cbird_amd.index import SearchParams
    from cbird_amd.video import VideoSearchParams, video_segments as segments_of_lists

    index, media = handle_of(gpu, clips)
    p = VideoSearchParams(algo=SearchParams.AlgoVideo, dctThresh=5, skipFrames=0, minFramesMatched=3)
    pairs = [(9, 7), (7, 9), (4, 4), (1, 12)]
    for got in (index.segments(pairs, p), index.segments(pairs, p, min_frames=3),
                segments_of_lists(clips, [(a - 1, b - 1) for a, b in pairs], 5, 0, min_frames=3)):
        for r, (a, b) in zip(got, pairs):
            s, segs, frames, dframes, dist, seg = SR.segments(clips[a - 1], clips[b - 1], 5, 0, 15, 3, 4)
            assert {k: getattr(r, k) for k in SR.SUMMARY_FIELDS} == s
            assert [vars(g) for g in r.segments] == segs
            assert (r.frames.tolist(), r.dst_frames.tolist(), r.distances.tolist(), r.segment_of.tolist()) == \
                (frames.tolist(), dframes.tolist(), dist.tolist(), seg.tolist())
            assert r.match_range() == (s["src_in"], s["dst_in"], s["len"])
            assert [vars(g) for g in r.cut_list()] == SR.cut_list(segs)
    assert got[0].percent() == 100 and got[0].n_segments >= 1 and got[3].n_segments == 0
    bare = index.segments(pairs, p, maps=False)
    assert [b.frames for b in bare] == [None] * 4 and [b.segments for b in bare] == [g.segments for g in got]
    assert index.segments([], p) == []
    one = index.segments(pairs, p, max_segments=1, tol=0, min_frames=1)
    want = SR.segments(clips[8], clips[6], 5, 0, 0, 1, 1)
    assert [vars(g) for g in one[0].segments] == want[1] and one[0].n_aligned == want[0]["n_aligned"]
    groups = [[media[8], media[6]], [media[6], media[8]]]
    video_segments(index, groups, p)
    assert groups[0][1].aligned == 100 and groups[0][1].segments.segments == got[0].segments
    assert groups[1][1].aligned == got[1].percent() < 100


def test_error_codes(gpu, lib, clips):
    from cbird_amd import _lib

    f, h, o = table(clips[:2])
    p = np.array([[0, 1]], np.uint32)
    sums = np.full(1, -1, np.int64).repeat(6).view(VSEGMENTS_DTYPE)
    segs = np.full(4, -1, np.int64).repeat(4).view(VSEGMENT_DTYPE)
    offs = np.full(3, 77, np.uint64)
    m = np.zeros(100, VSEGMENT_FRAME_DTYPE)

    def call(frames=f.ctypes.data, hashes=h.ctypes.data, voff=o.ctypes.data, n_videos=2, pairs=p.ctypes.data, n_pairs=1,
             skip=0, tol=15, min_frames=3, max_segments=4, s=sums.ctypes.data, g=segs.ctypes.data, map_=m.ctypes.data,
             cap=100, offsets=offs.ctypes.data, device=0):
        return lib.cbh_video_segments(device, frames, hashes, voff, n_videos, pairs, n_pairs, 5, skip, tol, min_frames,
                                      max_segments, s, g, map_, cap, offsets)

    falls = f.copy()
    falls[3] = falls[2] - 1  # a frame number that falls inside a named video
    for bad in (dict(frames=None), dict(hashes=None), dict(voff=None), dict(pairs=None), dict(s=None), dict(g=None),
                dict(offsets=None), dict(skip=-1), dict(n_videos=1), dict(tol=-1), dict(min_frames=0), dict(max_segments=0),
                dict(max_segments=17), dict(frames=falls.ctypes.data)):
        assert call(**bad) == _lib.CBH_E_INVAL, bad
        assert lib.cbh_last_error()  # (a text says which)
    assert call(device=99) == _lib.CBH_E_NODEVICE
    untouched = (np.full(6, -1, np.int64).tobytes(), np.full(16, -1, np.int64).tobytes())
    assert (sums.tobytes(), segs.tobytes()) == untouched and offs.tolist() == [77, 77, 77]  # nothing was written
    assert call(n_pairs=0) == 0 and offs.tolist() == [0, 77, 77]
    assert call(n_pairs=0, pairs=None, s=None, g=None, map_=None, offsets=None, frames=None, hashes=None) == 0
    assert call(map_=None, offsets=None) == 0 and int(sums[0]["n_src"]) == len(clips[0][0])
    assert call(max_segments=16, g=np.zeros(16, VSEGMENT_DTYPE).ctypes.data, tol=0, min_frames=1) == 0
    falling = np.array([0, 70, 60], np.uint64)
    assert call(voff=falling.ctypes.data) == _lib.CBH_E_INVAL
    equal = f.copy()
    equal[3] = equal[2]  # equal frame numbers do not fall
    assert call(frames=equal.ctypes.data) == 0

    index, _ = handle_of(gpu, clips[:3])
    ids = np.array([1, 2], np.uint32)
    unknown = np.array([2, 9], np.uint32)
    sums2 = np.full(2, -1, np.int64).repeat(6).view(VSEGMENTS_DTYPE)
    segs2 = np.zeros(8, VSEGMENT_DTYPE)
    offs[:] = 77

    def vcall(handle=index.handle, src=ids.ctypes.data, dst=ids.ctypes.data, n=2, tol=15):
        return lib.cbh_vidx_segments(handle, src, dst, n, 5, 0, tol, 3, 4, sums2.ctypes.data, segs2.ctypes.data, None, 0,
                                     offs.ctypes.data)

    assert vcall(dst=unknown.ctypes.data) == _lib.CBH_E_INVAL  # an id the handle does not hold
    assert sums2.tobytes() == np.full(12, -1, np.int64).tobytes() and offs.tolist() == [77, 77, 77]
    assert vcall(handle=None) == _lib.CBH_E_INVAL and vcall(src=None) == _lib.CBH_E_INVAL and vcall(tol=-1) == _lib.CBH_E_INVAL
    assert vcall(n=0, src=None, dst=None) == 0
    assert vcall() == 0 and offs.tolist() == [0, 70, 70 + len(clips[1][0])]


def test_every_allocation_may_be_refused(gpu, lib, clips):
    """the walk of tests/test_error_paths.py: every refused call returns CBH_E_NOMEM and leaves no device memory behind,
    and the handle gives the same answer afterwards"""
    from cbird_amd import _lib

    index, _ = handle_of(gpu, clips)
    pairs = ALL_PAIRS[:30]
    want = model(clips, pairs, PAR, key="clips")
    same(vidx_find(lib, index, pairs, PAR), want)
    refused = 0
    for k in range(100):
        live0, fired0 = _tuning(lib, b"arena_live_bytes"), _tuning(lib, b"fault_fired")
        lib.cbh_set_tuning(b"fault_alloc_after", k)
        try:
            rc = vidx_find(lib, index, pairs, PAR, maps=False)[0]
        finally:
            lib.cbh_set_tuning(b"fault_alloc_after", -1)
        if _tuning(lib, b"fault_fired") == fired0:
            assert rc == 0
            break
        refused += 1
        assert rc == _lib.CBH_E_NOMEM, (k, rc)
        assert _tuning(lib, b"arena_live_bytes") == live0, k
        same(vidx_find(lib, index, pairs, PAR), want)
    else:
        pytest.fail("the call never ran out of allocations to refuse")
    assert refused == 8  # source views, destination views, tables, state, difference arrays, summaries, segments, map
