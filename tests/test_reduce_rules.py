"""The video and keypoint-vote reductions (cbird_amd/csrc/reduce.hip: K8 k_video_winners / k_video_score, K5
k_fdct_pairs / runs / score) on cases that sit on a rule's edge (tests/reduce_rules.py): the plain model against the C
oracle on the CPU, and against findVideo / find_videos_batch / DctFeaturesIndex.find / find_batch on the GPU, through
the device reduction, the host reduction and the shipped choice between them.  Exact integer equality throughout."""
import warnings

import numpy as np
import pytest

import reduce_rules as R

VIDEO = {f.__name__: f for f in R.VIDEO_FIXTURES}
VOTE = {f.__name__: f for f in R.VOTE_FIXTURES}


@pytest.fixture(scope="module")
def fixtures():
    """every fixture with the true model's answer, computed once"""
    out = {}
    for name, build in {**VIDEO, **VOTE}.items():
        fx = build()
        out[name] = (fx, R.video_results(fx) if name in VIDEO else R.vote_results(fx))
    return out


@pytest.fixture(scope="module")
def vorc():
    from oracle import VideoOracle

    return VideoOracle()


# ---- CPU ---------------------------------------------------------------------------------------------------------
def test_every_target_holds_on_the_true_model(fixtures):
    """the builders assert their targets themselves; here: every fixture builds, states a target, stays small"""
    assert set(fixtures) == set(VIDEO) | set(VOTE)
    for name, (fx, want) in fixtures.items():
        assert fx.name == name and fx.target, name
        if "results" in fx.target:
            assert want == fx.target["results"], name
        if name in VIDEO and name != "dense_static":
            for sc in fx.scenes:
                assert len(sc.index) <= 36 and all(len(v[1]) <= 102 for v in sc.index + sc.needles), name
    hashes = [R.base(i) for i in range(126)]
    assert all(R.popc(h) == 32 for h in hashes)
    assert min(R.hamm64(a, b) for i, a in enumerate(hashes) for b in hashes[:i]) >= 24


def test_every_variant_is_killed(fixtures):
    """each wrong form of a rule changes the model's answer on the fixtures KILLS names for it: a kernel with that
    mistake could not pass them"""
    assert set(R.KILLS) == set(R.VIDEO_VARIANTS) | set(R.VOTE_VARIANTS)
    for variant, names in R.KILLS.items():
        assert names, variant
        for name in names:
            fx, want = fixtures[name]
            assert (name in VIDEO) == (variant in R.VIDEO_VARIANTS), (variant, name)
            got = R.video_results(fx, variant) if name in VIDEO else R.vote_results(fx, variant)
            assert got != want, (variant, name)


@pytest.mark.parametrize("name", list(VIDEO))
def test_video_oracle_equals_model(fixtures, vorc, name):
    fx, want = fixtures[name]
    for sc, want_sc in zip(fx.scenes, want):
        p = sc.params
        entries = vorc.build_entries(sc.index, p.skip)
        assert [(int(v), int(f), int(h)) for v, f, h in zip(*entries[:3])] == R.video_entries(sc.index, p.skip)
        for (nid, frames, hashes), w in zip(sc.needles, want_sc):
            got = vorc.find_video(entries, frames, np.array(hashes, np.uint64), nid, p.thresh, p.skip, p.vfm, p.vfn,
                                  filter_self=p.filter_self)
            assert got == w, (name, sc.note, nid)


@pytest.mark.parametrize("name", list(VOTE))
def test_vote_oracle_equals_model(fixtures, orc, name):
    fx, want = fixtures[name]
    for sc, want_sc in zip(fx.scenes, want):
        ids = np.array([m for m, _h in sc.live_rows], np.uint32)
        hashes = np.array([h for _m, h in sc.live_rows], np.uint64)
        for (nid, hs), w in zip(sc.needles, want_sc):
            gi, gs = orc.fdct_find(hashes, ids, np.array(hs, np.uint64), nid, sc.thresh)
            assert list(zip(gi.tolist(), gs.tolist())) == w, (name, nid)


# ---- GPU ---------------------------------------------------------------------------------------------------------
class _Media:
    def __init__(self, video):
        from cbird_amd.video import VideoIndex

        self.id, self.path, self.dctHash = video[0], f"v{video[0]}", 0
        self.videoIndex = VideoIndex(list(video[1]), [int(h) for h in video[2]])


def _video_index(scene):
    from cbird_amd.video import DctVideoIndex

    idx = DctVideoIndex()
    for op, arg in scene.steps:
        if op == "add":
            idx.add([_Media(v) for v in arg])
        else:
            idx.remove(arg)
    assert idx.count() == len(scene.index)
    return idx


def _video_params(p):
    from cbird_amd.video import VideoSearchParams

    return VideoSearchParams(dctThresh=p.thresh, skipFrames=p.skip, minFramesMatched=p.vfm, minFramesNear=p.vfn,
                             filterSelf=p.filter_self)


def _vkey(r):
    return [(x.mediaId, x.score, x.range.srcIn, x.range.dstIn, x.range.len) for x in r]


def _run_video(fx, want):
    """every scene of a fixture as one batch and needle by needle: (batch, singles), each checked against the model"""
    for sc, want_sc in zip(fx.scenes, want):
        idx, p = _video_index(sc), _video_params(sc.params)
        needles = [_Media(nd) for nd in sc.needles]
        batch = [_vkey(r) for r in idx.find_videos_batch(needles, p)]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # "needle video index is empty" for the needle without frames
            singles = [_vkey(idx.findVideo(m, p)) for m in needles]
        assert batch == want_sc, (fx.name, sc.note, "batch")
        assert singles == want_sc, (fx.name, sc.note, "single")
        assert batch == singles


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VIDEO))
def test_gpu_video_fixture(gpu, fixtures, reduce_path, name):
    _run_video(*fixtures[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VIDEO))
def test_gpu_video_fixture_auto_route(gpu, fixtures, name):
    """both knobs at 0: a single needle reduces on the host, a batch on the device; they agree with the model"""
    from cbird_amd import _lib

    L = _lib.lib()
    assert L.cbh_set_tuning(b"video_host_reduce", 0) == 0
    _run_video(*fixtures[name])


def _vote_index(gpu, scene):
    idx = gpu.DctFeaturesIndex()
    idx.load_flat(np.array([h for _m, h in scene.rows], np.uint64), np.array([m for m, _h in scene.rows], np.uint32))
    idx.remove(scene.removed)
    assert idx.count() == len(scene.rows)
    return idx


def _run_vote(gpu, fx, want):
    for sc, want_sc in zip(fx.scenes, want):
        idx, p = _vote_index(gpu, sc), gpu.SearchParams(dctThresh=sc.thresh)
        needles = [gpu.Media(id=nid, keyPointHashes=list(hs)) for nid, hs in sc.needles]
        batch = [[(m.mediaId, m.score) for m in r] for r in idx.find_batch(needles, p)]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # "needle has no hashes"
            singles = [[(m.mediaId, m.score) for m in idx.find(nd, p)] for nd in needles]
        assert batch == want_sc, (fx.name, "batch")
        assert singles == want_sc, (fx.name, "single")


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in VOTE if n != "cut_of_ten"])
def test_gpu_vote_fixture(gpu, fixtures, reduce_path, name):
    _run_vote(gpu, *fixtures[name])


@pytest.mark.gpu
def test_gpu_vote_cut_of_ten_on_every_scan(gpu, fixtures, scan_path, reduce_path):
    _run_vote(gpu, *fixtures["cut_of_ten"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VOTE))
def test_gpu_vote_fixture_auto_route(gpu, fixtures, name):
    from cbird_amd import _lib

    assert _lib.lib().cbh_set_tuning(b"fdct_host_vote", 0) == 0
    _run_vote(gpu, *fixtures[name])


@pytest.mark.gpu
def test_gpu_zero_needle_hash_on_every_scan(gpu, fixtures, scan_path):
    """a needle hash of 0 is searched like any other by findVideo and the vote (batch_shapes, batch_of_needles), while
    every scan kernel skips it for DctHashIndex::find: its records come from a pass of their own behind whichever
    kernel ran -- once, not twice"""
    _run_video(*fixtures["batch_shapes"])
    _run_vote(gpu, *fixtures["batch_of_needles"])


@pytest.mark.gpu
def test_gpu_zero_needle_hash_in_its_bucket(gpu, vorc, reduce_path):
    """`-p.vradix 2`: the zero needle frame sees 0x79 (5 bits from it, bits 1..2 clear like its own) and not 0x1f"""
    from cbird_amd.video import DctVideoIndex

    index = [R._video(61, [(0, R.base(R.PAD)), (20, 0x1F), (30, R.base(100)), (40, R.base(101)), (400, R.base(R.PAD))]),
             R._video(62, [(0, R.base(R.PAD)), (12, 0x79), (400, R.base(R.PAD))])]
    needle = R._padded(5, 10, [(0, R.base(100)), (1, 0), (2, R.base(101))])
    other = R._padded(6, 10, [(0, R.base(101))])
    p = R.VParams(thresh=6, skip=10)
    entries = vorc.build_entries(index, p.skip)
    for radix, want in ((0, [(61, 67, 10, 30, 10), (62, 0, 11, 12, 0)]), (2, [(61, 50, 10, 30, 10), (62, 0, 11, 12, 0)])):
        assert vorc.find_video(entries, needle[1], np.array(needle[2], np.uint64), 5, p.thresh, p.skip, p.vfm, p.vfn,
                               radix=radix) == want
        if radix == 0:
            assert R.find_video(index, needle, p) == want
        idx = DctVideoIndex(radix_compat=True)
        idx.add([_Media(v) for v in index])
        vp = _video_params(p)
        vp.videoRadix = radix
        assert _vkey(idx.findVideo(_Media(needle), vp)) == want, radix
        assert _vkey(idx.find_videos_batch([_Media(other), _Media(needle)], vp)[1]) == want, radix


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["distance_ties", "dense_static", "batch_of_needles"])
def test_gpu_fixture_on_a_sharded_handle(gpu, fixtures, reduce_path, name):
    """five logical shards: the reductions read the merged record block"""
    from cbird_amd import _lib

    _lib.set_default_sharding((1, 5))
    try:
        if name in VIDEO:
            _run_video(*fixtures[name])
        else:
            _run_vote(gpu, *fixtures[name])
    finally:
        _lib.set_default_sharding(None)
