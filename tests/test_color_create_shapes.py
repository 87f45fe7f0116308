"""ColorDescriptor::create on the device at every images-per-wave shape (k_cdw_round<G>, G = 1, 2, 4, 8, 16, 21), at the
tile and quarter-row edges of its two chain loops, with odd and ragged tails for the kernels behind it, in chunks, from
padded rows and from device memory: byte for byte against oracle/colordesc_oracle.c.  The images are
tests/color_create_cases.py's; the CPU tests here keep them on their edges, the GPU tests prove through
"color_create_group_last" which instantiation they ran."""
import time

import numpy as np
import pytest

import color_create_cases as S


# ---- CPU: the fixtures are what they claim to be ---------------------------------------------------------------------
def _tail_call():
    """65 images for G = 1: more than one wave of the lane-per-image kernels (k_cdw_post, k_cdw_finish: 64), the 64th
    image "few", the 65th invalid"""
    valid = [c for c in S.RAGGED if c.valid and c is not S.big()]
    few = [c for c in valid if c.palette == "few"]
    imgs = [valid[i % len(valid)] for i in range(63)] + [few[3], S.lit(64, 48, 31, "few", seed=3)]
    assert len(imgs) == 65 and imgs[63].palette == "few" and imgs[63].valid and not imgs[64].valid
    return imgs


def _chunk_call():
    """150 images = chunks of 64, 64 and 22 at "color_create_chunk_mb" 1; the 256 x 192 image in every chunk (it sets each
    chunk's cap to 49152 slots), the rest RAGGED's other images repeated"""
    rest = [c for c in S.RAGGED if c is not S.big()]
    imgs = [rest[i % len(rest)] for i in range(150)]
    for at in (5, 64 + 63, 128 + 9):
        imgs[at] = S.big()
    return imgs


def test_fixtures_have_their_sample_counts():
    cases = list(dict.fromkeys(S.RAGGED + S.ALL_INVALID + _tail_call()))
    assert len(S.RAGGED) == 47 and len(set(map(id, S.RAGGED))) == 47 and len(S.ALL_INVALID) == 26
    for c in cases:
        desc, st = S.want(c)
        assert st[:3] == (c.cols, c.rows, c.N), (c.name, st)   # no resize, exactly N samples
        assert (desc is not None) == (c.N >= 32) == c.valid, (c.name, st)
    # every edge N is in RAGGED, in both palettes where the fill repeats it
    assert {c.N for c in S.RAGGED if c.name.startswith("lit")} == set(S.EDGE_N)
    assert sorted(S.EDGE_N) == [0, 31, 32, 33, 48, 49, 63, 64, 65, 66, 80, 81, 113, 127, 128, 129, 130, 192, 193, 256, 257,
                                1000, 1025]
    by = {c.palette for c in S.RAGGED}
    assert by == {"spread", "few", "grey", "random", "photo", "black"}
    # the figures the list was designed around
    grey = [c for c in S.RAGGED if c.palette == "grey"]
    tiny = [c for c in S.RAGGED if (c.cols, c.rows) == (16, 12)]
    assert len(grey) == 1 and grey[0].N == 200
    assert len(tiny) == 2 and all(c.N == 141 for c in tiny)
    assert S.big().N == 31543 and -(-S.big().N // 64) == 493 and sum(c is S.big() for c in S.RAGGED) == 1
    assert sum((c.cols, c.rows) == (100, 100) for c in S.RAGGED) == 1
    assert [c.N for c in S.ALL_INVALID[:21]] == [0] * 21 and all(c.valid for c in S.ALL_INVALID[21:])
    # the grey cut: 15 is dropped, 16 is kept
    lo, hi = np.full((64, 48, 3), 15, np.uint8), np.full((64, 48, 3), 16, np.uint8)
    assert S.oracle().create(lo)[1][2] == 0 and S.oracle().create(hi)[1][2] == int((S.oracle().ellipse_mask(48, 64) == 255).sum())


def test_few_palette_ends_with_at_most_five_colours():
    few = [c for c in S.RAGGED + S.ALL_INVALID if c.palette == "few" and c.valid]
    assert len(few) >= 15
    for c in few + [c for c in S.RAGGED if c.palette == "grey"]:
        desc, _ = S.want(c)
        assert int(desc[256]) + 1 <= 5, (c.name, int(desc[256]))   # numColors holds the index of the last colour
    spread = [S.want(c)[0] for c in S.RAGGED if c.palette == "spread" and c.valid]
    assert max(int(d[256]) + 1 for d in spread) > 16              # ... and the other palette fills the clusters


def test_ragged_order():
    R = S.RAGGED
    n = len(R)
    assert n % 2 == 1 and R[-1].valid and R[-1].palette == "few"   # the odd image of the two-per-wave kernels is real work
    for G in S.GROUPS[1:]:
        assert n % G != 0                                          # a partly filled last wave
    where = S.wave_slots(n, G=1)
    assert where == [(i, 0, 1) for i in range(n)]
    for G in (4, 8, 21):
        slots = {slot for (wave, slot, held), c in zip(S.wave_slots(n, G), R) if not c.valid and held == G}
        assert 0 in slots and G - 1 in slots and any(0 < s < G - 1 for s in slots), (G, slots)
    at = R.index(S.big())
    for G in (4, 8, 16, 21):
        ws = S.wave_slots(n, G)
        mates = [c for c, w in zip(R, ws) if w[0] == ws[at][0] and c is not S.big()]
        assert any(c.N == 32 for c in mates) and any(not c.valid for c in mates), G
    # every image's n is far below the wave's nmax next to the large one
    assert all(c.N * 4 < S.big().N for c in R if c is not S.big())


def test_rotations():
    for G in S.GROUPS:
        rots = S.rotations(S.RAGGED, G)
        want = list(dict.fromkeys((0, -(-G // 3), -(-2 * G // 3))))
        assert [r.index(S.RAGGED[0]) for r in rots] == [(-k) % 47 for k in want]
        assert all(sorted(map(id, r)) == sorted(map(id, S.RAGGED)) for r in rots)
    assert len(S.rotations(S.RAGGED, 1)) == 2 and len(S.rotations(S.RAGGED, 21)) == 3


def test_the_calls_built_from_the_list():
    t = _chunk_call()
    assert len(t) == 150 and [i for i, c in enumerate(t) if c is S.big()] == [5, 127, 137]
    assert {i // 64 for i, c in enumerate(t) if c is S.big()} == {0, 1, 2}
    # 64 MB (the least the launcher accepts) / 33 bytes per slot / 49152 slots = 41 -> the floor of 64 images per chunk
    assert max((64 << 20) // (33 * 49152), 64) == 64
    _tail_call()


def test_color_create_group_refuses_values_it_does_not_know():
    """"color_create_group" takes 0 and the six G that exist; anything else is refused and leaves the knob as it was (a
    test that means to force an instantiation must not silently run another).  "color_create_group_last" is read-only."""
    from cbird_amd import _lib

    L = _lib.lib()
    try:
        assert S.tuning(L, b"color_create_group") == 0              # as shipped: by the chunk's size
        for good in S.GROUPS + (0, 16):
            assert L.cbh_set_tuning(b"color_create_group", good) == _lib.CBH_OK
            assert S.tuning(L, b"color_create_group") == good
        for bad in (-1, 3, 5, 6, 7, 9, 15, 17, 20, 22, 32, 64, 1 << 20):
            assert L.cbh_set_tuning(b"color_create_group", bad) == _lib.CBH_E_INVAL
            assert S.tuning(L, b"color_create_group") == 16
        last = S.tuning(L, b"color_create_group_last")
        assert last in (0,) + S.GROUPS
        for v in (0, 1, 21):
            assert L.cbh_set_tuning(b"color_create_group_last", v) == _lib.CBH_E_INVAL
        assert S.tuning(L, b"color_create_group_last") == last
    finally:
        assert L.cbh_set_tuning(b"color_create_group", 0) == _lib.CBH_OK


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def create(gpu):
    """run(cases or packed batch, group=G, expect=G', ...) -> (descs [n, 258], ok [n]) with "color_create_group" at G for
    the call; asserts that the last chunk launched k_cdw_round<expect> (expect defaults to G).  The knobs go back to
    their defaults whatever happens."""
    from cbird_amd import _lib

    L = _lib.lib()

    def run(batch, group, expect=None, dev=False, pad=0, ch=3, chunk_mb=None):
        packed = S.pack([c.img for c in batch], pad=pad) if isinstance(batch, list) else batch
        assert L.cbh_set_tuning(b"color_create_group", group) == 0
        if chunk_mb is not None:
            assert L.cbh_set_tuning(b"color_create_chunk_mb", chunk_mb) == 0
        got = (S.run_dev if dev else S.run_host)(L, packed, ch)
        assert S.tuning(L, b"color_create_group_last") == (expect or group), (group, expect)
        return got

    try:
        yield run
    finally:
        L.cbh_set_tuning(b"color_create_group", 0)
        L.cbh_set_tuning(b"color_create_chunk_mb", S.CHUNK_MB_DEFAULT)


def _same(got, cases, G, tag):
    """== on all 258 bytes and on ok, for every image; a difference names the smallest (position, slot in its wave, N)"""
    descs, ok = got
    wd, wok = S.want_arrays(cases)
    bad = np.flatnonzero((descs != wd).any(axis=1) | (ok != wok))
    if len(bad):
        ws = S.wave_slots(len(cases), G)
        lines = [f"  image {i}: wave {ws[i][0]} slot {ws[i][1]} of {ws[i][2]}, N={cases[i].N} {cases[i].name}: ok {ok[i]} want "
                 f"{wok[i]}, {int((descs[i] != wd[i]).sum())} bytes differ (first at {int(np.argmax(descs[i] != wd[i]))})"
                 for i in bad[:12]]
        raise AssertionError(f"G={G} {tag}: {len(bad)} of {len(cases)} images differ from the oracle\n" + "\n".join(lines))


_WARM = []


def _warm_batch():
    """eight 256 x 192 random images: what the scratch blocks hold before the ragged batch gets them"""
    if not _WARM:
        _WARM.append(S.pack([S.whole(256, 192, 100 + i).img for i in range(8)]))
    return _WARM[0]


@pytest.mark.gpu
@pytest.mark.parametrize("G", S.GROUPS)
def test_every_group_size_on_the_ragged_batch(create, G):
    """RAGGED at each of its rotations, then ALL_INVALID, on k_cdw_round<G>.  Before the first ragged call one call with
    eight full 256 x 192 images runs at the same G, so that the cached scratch blocks the ragged batch receives hold
    another batch's samples and distances past each image's n rather than fresh zeros -- best effort: the allocator may
    hand out other blocks (the batches differ in size), and nothing here can tell which it did."""
    t0 = time.perf_counter()
    _, ok = create(_warm_batch(), G)
    assert (ok == 1).all()
    for r, cases in enumerate(S.rotations(S.RAGGED, G)):
        _same(create(cases, G), cases, G, f"RAGGED rotation {r}")
    _same(create(S.ALL_INVALID, G), S.ALL_INVALID, G, "ALL_INVALID")
    print(f"G={G}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.gpu
def test_group_sizes_agree_with_each_other(create):
    """the six instantiations return identical arrays for RAGGED: a second witness that does not involve the oracle, and
    one that pins a failure of the test above on one G"""
    packed = S.pack([c.img for c in S.RAGGED])
    got = {G: create(packed, G) for G in S.GROUPS}
    for G in S.GROUPS[1:]:
        diff = np.flatnonzero((got[G][0] != got[1][0]).any(axis=1) | (got[G][1] != got[1][1]))
        assert len(diff) == 0, (G, diff.tolist(), [S.RAGGED[i].name for i in diff])


_POOL = {}


def _pool():
    """32769 random 16 x 12 images (141 samples each), one block; a batch is a prefix of it"""
    if not _POOL:
        _POOL["px"] = np.random.default_rng(2048).integers(40, 256, (32769, 12, 16, 3), dtype=np.uint8)
        _POOL["want"] = {}
    return _POOL["px"]


def _pool_want(i):
    w = _POOL["want"].get(i)
    if w is None:
        w, st = S.oracle().create(_pool()[i])
        assert w is not None and st[:3] == (16, 12, 141)
        _POOL["want"][i] = w
    return w


def _threshold_sample(n, G):
    """every image of the first and of the last wave, both sides of 16 wave boundaries spread over the batch, every 4th"""
    waves = -(-n // G)
    pick = set(range(min(G, n))) | set(range((waves - 1) * G, n)) | set(range(0, n, 4))
    for k in np.unique(np.linspace(1, waves - 1, 16).astype(np.int64)):
        pick |= {int(k) * G - 1, int(k) * G}
    pick |= {63, 64, n - 1, n - 2}          # the lane-per-image kernels' wave edge; the last pair of the two-per-wave ones
    return sorted(i for i in pick if 0 <= i < n)


@pytest.mark.gpu
def test_the_shipped_rule_at_its_thresholds(create):
    """"color_create_group" 0: the launcher's own rule, at the first batch size that takes each G.  Sampled against the
    oracle (_threshold_sample); and, since a batch is a prefix of the next one and descriptors do not depend on the
    batch, EVERY image of a batch against the same image in the next size's result -- computed by another G."""
    from cbird_amd import _lib

    L = _lib.lib()
    px = _pool()
    prev = None
    for n, G in ((2048, 1), (2049, 2), (4097, 4), (8193, 8), (16385, 16), (32769, 21)):
        t0 = time.perf_counter()
        per = 12 * 16 * 3                    # 576: a multiple of 16, so the images are packed back to back
        packed = (px[:n].reshape(-1), np.arange(n, dtype=np.uint64) * np.uint64(per), np.full(n, 16, np.uint32),
                  np.full(n, 12, np.uint32), np.full(n, 48, np.uint32))
        descs, ok = create(packed, 0, expect=G)
        assert S.tuning(L, b"color_create_group") == 0
        assert (ok == 1).all(), (n, np.flatnonzero(ok != 1)[:8])
        for i in _threshold_sample(n, G):
            assert (descs[i] == _pool_want(i)).all(), (n, G, i, i // G, i % G)
        if prev is not None:
            diff = np.flatnonzero((descs[: len(prev)] != prev).any(axis=1))
            assert len(diff) == 0, (n, G, diff[:8].tolist())
        prev = descs
        print(f"{n} images, G={G}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.gpu
def test_chunked_batches_equal_one_piece(create):
    """"color_create_chunk_mb" 1 (taken as 64 MB = 64 images at 49152 slots each): chunks of 64, 64 and 22 images, each with
    its own cap, descriptors and flags at d_descs + i0 * 258 and d_ok + i0, the scratch blocks of the chunk before"""
    cases = _chunk_call()
    packed = S.pack([c.img for c in cases])
    one = create(packed, 0, expect=1)
    cut = create(packed, 0, expect=1, chunk_mb=1)
    assert (cut[0] == one[0]).all() and (cut[1] == one[1]).all()
    _same(cut, cases, 1, "in chunks of 64")       # every image, so 0, 63, 64, 65, 127, 128 and 149 among them
    _same(one, cases, 1, "in one piece")
    cut8 = create(packed, 8, chunk_mb=1)          # 64 = 8 whole waves per chunk, the last chunk 2 waves + 6 images
    assert (cut8[0] == one[0]).all() and (cut8[1] == one[1]).all()


@pytest.mark.gpu
def test_padded_rows_and_device_input(create):
    """rows 5 bytes longer than their pixels (the padding and the gaps between images hold 255: read as pixels they would
    be white samples), through cbh_color_descriptors and, from torch tensors, cbh_color_descriptors_dev; BGR and BGRA"""
    R = S.RAGGED
    rng = np.random.default_rng(4)
    bgra = [np.dstack([c.img, rng.integers(0, 256, c.img.shape[:2], dtype=np.uint8)]) for c in R]
    for G in (1, 8):
        _same(create(R, G, pad=5), R, G, "host, padded rows")
        _same(create(R, G, dev=True), R, G, "device, BGR")
        _same(create(R, G, dev=True, pad=5), R, G, "device, BGR, padded rows")
        _same(create(S.pack(bgra), G, dev=True, ch=4), R, G, "device, BGRA")
        _same(create(S.pack(bgra, pad=5), G, ch=4), R, G, "host, BGRA, padded rows")


@pytest.mark.gpu
def test_more_than_one_wave_of_the_lane_per_image_kernels(create):
    """65 images at G = 1: k_cdw_post and k_cdw_finish (64 images per wave) run a second wave of one image, and it is an
    invalid one; the image before it has five colours (empty clusters in k_cdw_post's last lane); k_cdw_update and
    k_cdw_freq (two per wave) end on a single image"""
    cases = _tail_call()
    _same(create(cases, 1), cases, 1, "65 images")
    _same(create(cases[:64], 1), cases[:64], 1, "64 images")
