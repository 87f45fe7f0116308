"""GPU: alignSpatially and alignTemporally on the device (cbird_amd/csrc/align.hip) against the numpy model
(tests/alignment_rules.py) with no tolerance: the full 289-entry tables, the records, the means and the cells; host and
device entries, a side stream, padded rows, odd offsets and guard words around every output."""
import ctypes as C

import numpy as np
import pytest

import alignment_rules as A
import difference_rules as R

pytestmark = pytest.mark.gpu
GUARD, PAD, WORD = 0x5A, 0xA5, 0x5A5A5A5A
SFIELDS = ["min_x", "min_y", "min_sad", "sad_at_zero"]
TFIELDS = ["placement", "offset", "min_mean", "start_mean"]


def _tuning(L, key):
    v = C.c_longlong(0)
    assert L.cbh_get_tuning(key, C.byref(v)) == 0
    return v.value


@pytest.fixture(scope="module")
def lib(gpu):
    from cbird_amd import _lib

    return _lib.lib()


def _ch(im):
    return 1 if im.ndim == 2 else im.shape[2]


def _ptr(a):
    return None if a is None else a.ctypes.data


def pack_ragged(imgs, rng, gap=40):
    """images with padded rows, gaps and odd offsets; everything that is not a pixel is PAD (tests/test_difference.py)"""
    off, stride, pos = [], [], 1 + 2 * int(rng.integers(0, 4))
    for im in imgs:
        h, w = im.shape[:2]
        st = w * _ch(im) + int(rng.integers(0, 7))
        off.append(pos), stride.append(st)
        pos += st * h + int(rng.integers(0, gap))
    buf = np.full(pos + 32, PAD, np.uint8)
    for im, o, st in zip(imgs, off, stride):
        h, w = im.shape[:2]
        np.lib.stride_tricks.as_strided(buf[o:], (h, w * _ch(im)), (st, 1))[:] = im.reshape(h, w * _ch(im))
    return (buf, np.array(off, np.uint64), np.array([im.shape[1] for im in imgs], np.uint32),
            np.array([im.shape[0] for im in imgs], np.uint32), np.array(stride, np.uint32))


def pack_plain(imgs):
    from cbird_amd.quality import pack_images

    return pack_images([np.ascontiguousarray(im) for im in imgs])


def pack(imgs, ragged_seed):
    return pack_plain(imgs) if ragged_seed is None else pack_ragged(imgs, np.random.default_rng(ragged_seed))


_sources: dict = {}
_tables: dict = {}


def source(k, ch):
    """source k of A.SOURCE_SIZES in `ch` channels (a random alpha in the fourth): made once, never written to"""
    if (k, ch) not in _sources:
        w, h = A.SOURCE_SIZES[k]
        _sources[k, ch] = R.textured(w, h, 40 + k, ch)
    return _sources[k, ch]


def want_spatial(left, right):
    """the model's (table, record) of a pair: worked out once per distinct pair"""
    key = (left.shape, hash(left.tobytes()), right.shape, hash(right.tobytes()))
    if key not in _tables:
        _tables[key] = A.align_spatial(left, right)
    return _tables[key]


# ---- spatial ----------------------------------------------------------------------------------------------------------
def spatial_dev(L, left, rights, table=True, stream=None, ragged_seed=None):
    """-> (rc, records, tables or None); checks the guards itself"""
    import torch

    from cbird_amd.alignment import ALIGN_SPATIAL_DTYPE

    n = len(rights)
    lp = pack([left], None if ragged_seed is None else 99)
    rp = pack(rights, ragged_seed) if n else (np.zeros(16, np.uint8),) + (None,) * 4
    d_left = torch.from_numpy(lp[0]).cuda()
    d_rights = torch.from_numpy(rp[0]).cuda()
    d_res = torch.full((n * 16 + 64,), GUARD, dtype=torch.uint8, device="cuda")
    d_tab = torch.full((n * 289 + 16,), WORD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = L.cbh_align_spatial_dev(d_left.data_ptr() + int(lp[1][0]), left.shape[1], left.shape[0], int(lp[4][0]), _ch(left),
                                 d_rights.data_ptr(), n, _ptr(rp[1]), _ptr(rp[2]), _ptr(rp[3]), _ptr(rp[4]),
                                 _ch(rights[0]) if n else 3, d_res.data_ptr(), d_tab.data_ptr() if table else None, 0,
                                 stream.cuda_stream if stream else None)
    torch.cuda.synchronize()
    res, tab = d_res.cpu().numpy(), d_tab.cpu().numpy().view(np.uint32)
    assert (res[n * 16:] == GUARD).all() and (tab[n * 289:] == WORD).all()
    if not table or rc != 0:
        assert (tab == WORD).all()
    if rc != 0:
        assert (res == GUARD).all()
    return rc, res[:n * 16].view(ALIGN_SPATIAL_DTYPE), tab[:n * 289].reshape(n, 17, 17) if table else None


def spatial_host(L, left, rights, table=True):
    from cbird_amd.alignment import ALIGN_SPATIAL_DTYPE

    n = len(rights)
    left = np.ascontiguousarray(left)
    buf, off, w, h, st = pack_plain(rights) if n else (np.zeros(16, np.uint8),) + (None,) * 4
    res = np.full(n * 16 + 64, GUARD, np.uint8)
    tab = np.full(n * 289 + 16, WORD, np.uint32)
    rc = L.cbh_align_spatial(left.ctypes.data, left.shape[1], left.shape[0], left.shape[1] * _ch(left), _ch(left),
                             buf.ctypes.data, buf.size, n, _ptr(off), _ptr(w), _ptr(h), _ptr(st), _ch(rights[0]) if n else 3,
                             res.ctypes.data, tab.ctypes.data if table else None, 0)
    assert (res[n * 16:] == GUARD).all() and (tab[n * 289:] == WORD).all()
    if not table or rc != 0:
        assert (tab == WORD).all()
    return rc, res[:n * 16].view(ALIGN_SPATIAL_DTYPE), tab[:n * 289].reshape(n, 17, 17) if table else None


def check_spatial(what, left, rights, res, tab):
    assert len(res) == len(rights)
    for i, r in enumerate(rights):
        wtab, wrec = want_spatial(left, r)
        if tab is not None:
            assert (tab[i] == wtab).all(), (what, i, np.argwhere(tab[i] != wtab)[:4])
        for f in SFIELDS:
            assert int(res[i][f]) == wrec[f], (what, i, f, int(res[i][f]), wrec[f])


PAIRINGS = [(a, b) for a in (1, 3, 4) for b in (1, 3, 4)]


@pytest.mark.parametrize("lch,rch", PAIRINGS)
def test_spatial_equals_the_model_at_every_source_size(lib, lch, rch):
    """every source size as a right image (and, over the pairings, as the left one): 1 x 1, 3 x 5, the identity, one off
    it, 641 x 479 and the longest sides; the device entry on a side stream with padded rows and odd offsets, then the
    host entry"""
    import torch

    left = source(PAIRINGS.index((lch, rch)) % len(A.SOURCE_SIZES), lch)
    rights = [source(k, rch) for k in range(len(A.SOURCE_SIZES))]
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    rc, res, tab = spatial_dev(lib, left, rights, stream=side, ragged_seed=10 * lch + rch)
    assert rc == 0
    check_spatial("dev", left, rights, res, tab)
    rc, res2, none = spatial_dev(lib, left, rights, table=False)
    assert rc == 0 and none is None and res2.tobytes() == res.tobytes()
    rc, res3, tab3 = spatial_host(lib, left, rights)
    assert rc == 0 and res3.tobytes() == res.tobytes() and (tab3 == tab).all()


def test_spatial_batches_of_0_1_and_67(lib):
    pool = [R.textured(w, h, 60 + k) for k, (w, h) in enumerate([(3, 5), (17, 9), (40, 31), (64, 64), (5, 90)])]
    left = R.textured(33, 21, 59)
    rights = [pool[i % 5] for i in range(67)]
    for entry in (spatial_dev, spatial_host):
        rc, res, tab = entry(lib, left, rights)
        assert rc == 0
        check_spatial(entry.__name__, left, rights, res, tab)
        rc, res1, tab1 = entry(lib, left, rights[3:4])
        assert rc == 0 and res1.tobytes() == res[3:4].tobytes() and (tab1[0] == tab[3]).all()
        rc, res0, tab0 = entry(lib, left, [])  # (the helpers assert that every guard survived)
        assert rc == 0 and len(res0) == 0
    assert lib.cbh_align_spatial_dev(None, 5, 5, 15, 3, None, 0, None, None, None, None, 3, None, None, 0, None) == 0
    assert lib.cbh_align_spatial(None, 5, 5, 15, 3, None, 0, 0, None, None, None, None, 3, None, None, 0) == 0


def test_spatial_ties_extremes_and_planted_shifts(lib):
    row = np.array([10, 80, 160, 250], np.uint8)[np.arange(256) % 4]
    periodic = np.repeat(np.repeat(row[None, :], 256, axis=0)[:, :, None], 3, axis=2)
    cases = [("constant", np.full((5, 7, 3), 90, np.uint8), np.full((9, 4, 3), 100, np.uint8), (-8, -8, 240 * 240 * 30)),
             ("periodic", periodic, periodic, (-8, -8, 0)),
             ("extreme", np.zeros((2, 2, 3), np.uint8), np.full((3, 3, 3), 255, np.uint8), (-8, -8, 44064000))]
    for dx, dy in [(-8, -8), (8, 8), (-8, 8), (8, -8), (0, 0), (3, -5)]:
        l, r = A.planted(dx, dy, seed=3)
        cases.append((f"planted {dx} {dy}", l, r, (dx, dy, 0)))
    for name, left, right, (mx, my, sad) in cases:
        rc, res, tab = spatial_dev(lib, left, [right])
        assert rc == 0
        assert (int(res[0]["min_x"]), int(res[0]["min_y"]), int(res[0]["min_sad"])) == (mx, my, sad), name
        check_spatial(name, left, [right], res, tab)
    assert (tab == 0).sum() == 1  # (the last planted pair: one zero in its table)


# ---- temporal ---------------------------------------------------------------------------------------------------------
def temporal_dev(L, left, right, start, means=True, cells=True, stream=None, ragged_seed=None):
    import torch

    from cbird_amd.alignment import ALIGN_TEMPORAL_DTYPE

    nl, nw = len(left), len(right)
    p = max(nl - nw + 1, 1)
    lp, rp = pack(left, ragged_seed), pack(right, None if ragged_seed is None else ragged_seed + 1)
    d_l, d_r = torch.from_numpy(lp[0]).cuda(), torch.from_numpy(rp[0]).cuda()
    d_rec = torch.full((16 + 64,), GUARD, dtype=torch.uint8, device="cuda")
    d_means = torch.full((p + 16,), WORD, dtype=torch.int32, device="cuda")
    d_cells = torch.full((p * nw + 16,), WORD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = L.cbh_align_temporal_dev(d_l.data_ptr(), nl, _ptr(lp[1]), _ptr(lp[2]), _ptr(lp[3]), _ptr(lp[4]), _ch(left[0]),
                                  d_r.data_ptr(), nw, _ptr(rp[1]), _ptr(rp[2]), _ptr(rp[3]), _ptr(rp[4]), _ch(right[0]), start,
                                  d_rec.data_ptr(), d_means.data_ptr() if means else None,
                                  d_cells.data_ptr() if cells else None, 0, stream.cuda_stream if stream else None)
    torch.cuda.synchronize()
    rec, mm, cc = d_rec.cpu().numpy(), d_means.cpu().numpy().view(np.uint32), d_cells.cpu().numpy().view(np.uint32)
    assert (rec[16:] == GUARD).all() and (mm[p:] == WORD).all() and (cc[p * nw:] == WORD).all()
    if not means or rc != 0:
        assert (mm == WORD).all()
    if not cells or rc != 0:
        assert (cc == WORD).all()
    if rc != 0:
        assert (rec == GUARD).all()
    return rc, rec[:16].view(ALIGN_TEMPORAL_DTYPE)[0], mm[:p] if means else None, cc[:p * nw].reshape(p, nw) if cells else None


def temporal_host(L, left, right, start, means=True, cells=True):
    from cbird_amd.alignment import ALIGN_TEMPORAL_DTYPE

    nl, nw = len(left), len(right)
    p = max(nl - nw + 1, 1)
    lp, rp = pack_plain(left), pack_plain(right)
    rec = np.full(16 + 64, GUARD, np.uint8)
    mm = np.full(p + 16, WORD, np.uint32)
    cc = np.full(p * nw + 16, WORD, np.uint32)
    rc = L.cbh_align_temporal(lp[0].ctypes.data, lp[0].size, nl, _ptr(lp[1]), _ptr(lp[2]), _ptr(lp[3]), _ptr(lp[4]),
                              _ch(left[0]), rp[0].ctypes.data, rp[0].size, nw, _ptr(rp[1]), _ptr(rp[2]), _ptr(rp[3]),
                              _ptr(rp[4]), _ch(right[0]), start, rec.ctypes.data, mm.ctypes.data if means else None,
                              cc.ctypes.data if cells else None, 0)
    assert (rec[16:] == GUARD).all() and (mm[p:] == WORD).all() and (cc[p * nw:] == WORD).all()
    if not means or rc != 0:
        assert (mm == WORD).all()
    if not cells or rc != 0:
        assert (cc == WORD).all()
    return rc, rec[:16].view(ALIGN_TEMPORAL_DTYPE)[0], mm[:p] if means else None, cc[:p * nw].reshape(p, nw) if cells else None


def clip(n, seed, w=9, h=7, ch=3):
    return [R.textured(w, h, seed + k, ch) for k in range(n)]


def temporal_cases():
    """name -> (left frames, right frames, start)"""
    c = {}
    left = clip(64, 100)
    c["reference 64 / 5 / 30, planted at 41"] = (left, left[41:46], 30)
    c["planted at the start"] = (left, left[30:35], 30)
    c["planted at 0"] = (left, left[0:5], 30)
    c["other sizes and channel counts"] = (clip(64, 200, 13, 6, 4), clip(5, 231, 4, 11, 1), 30)
    c["1 x 1 against the longest side"] = (clip(9, 300, 1, 1, 1), clip(2, 303, 32767, 1, 3), 4)
    c["one placement"] = (clip(5, 400), clip(5, 402), 0)
    c["a window of one frame"] = (clip(7, 500), clip(1, 503), 3)
    c["a window of 64 frames"] = (clip(66, 600, 3, 5, 1), clip(64, 601, 3, 5, 1), 1)
    st = R.textured(8, 8, 700)
    c["a static clip stays at start"] = ([st] * 12, [R.textured(8, 8, 701)] * 3, 4)
    black = np.zeros((128, 128, 3), np.uint8)

    def ones(k):
        f = black.copy()
        f.reshape(-1)[:k] = 1
        return f

    c["equal integer means keep the earlier placement"] = ([ones(k) for k in (11, 10, 10, 30)], [black, black], 2)
    c["a mean equal to start's does not win"] = ([ones(k) for k in (10, 10, 11, 30)], [black, black], 1)
    c["black against white"] = ([black] * 3, [255 - black] * 2, 1)
    return c


TCASES = temporal_cases()
_tmodels: dict = {}


def want_temporal(name):
    if name not in _tmodels:
        _tmodels[name] = A.align_temporal(*TCASES[name])
    return _tmodels[name]


@pytest.mark.parametrize("name", list(TCASES))
def test_temporal_equals_the_model(lib, name):
    import torch

    left, right, start = TCASES[name]
    wcells, wmeans, wrec = want_temporal(name)
    side = torch.cuda.Stream()
    rc, rec, means, cells = temporal_dev(lib, left, right, start, stream=side, ragged_seed=7)
    assert rc == 0
    assert (cells == wcells).all() and (means == wmeans).all()
    for f in TFIELDS:
        assert int(rec[f]) == wrec[f], (f, int(rec[f]), wrec[f])
    rc, rec2, none, none2 = temporal_dev(lib, left, right, start, means=False, cells=False)
    assert rc == 0 and none is None and none2 is None and rec2.tobytes() == rec.tobytes()
    rc, rec3, means3, cells3 = temporal_host(lib, left, right, start)
    assert rc == 0 and rec3.tobytes() == rec.tobytes() and (means3 == means).all() and (cells3 == cells).all()
    rc, rec4, _, _ = temporal_host(lib, left, right, start, means=False, cells=False)
    assert rc == 0 and rec4.tobytes() == rec.tobytes()


def test_temporal_expectations_of_the_cases():
    """what the cases are there for, from the model (no device)"""
    assert want_temporal("reference 64 / 5 / 30, planted at 41")[2] == dict(
        placement=41, offset=11, min_mean=0, start_mean=int(want_temporal("reference 64 / 5 / 30, planted at 41")[1][30]))
    assert want_temporal("planted at the start")[2]["placement"] == 30 and want_temporal("planted at 0")[2]["offset"] == -30
    assert want_temporal("a static clip stays at start")[2]["placement"] == 4
    assert list(want_temporal("equal integer means keep the earlier placement")[1]) == [10, 10, 20]
    assert want_temporal("equal integer means keep the earlier placement")[2]["placement"] == 0
    assert want_temporal("a mean equal to start's does not win")[2]["placement"] == 1
    assert (want_temporal("black against white")[0] == 12533760).all()


# ---- arguments and refused allocations --------------------------------------------------------------------------------
def test_arguments(lib):
    from cbird_amd import _lib

    L, INVAL = lib, _lib.CBH_E_INVAL
    left = R.textured(23, 17, 1)
    rights = [R.textured(10, 7, 2), R.textured(31, 29, 3)]
    buf, off, w, h, st = pack_plain(rights)
    n = len(rights)
    res = np.zeros(n * 16, np.uint8)

    def spatial(lw=23, lh=17, lstride=69, lch=3, ch=3, n=n, w=w, h=h, stride=st, bytes_=buf.size, res=res):
        L.cbh_clear_error()
        rc = L.cbh_align_spatial(left.ctypes.data, lw, lh, lstride, lch, buf.ctypes.data, bytes_, n, _ptr(off), _ptr(w),
                                 _ptr(h), _ptr(stride), ch, _ptr(res), None, 0)
        if rc == INVAL:
            assert L.cbh_last_error().decode().startswith("align spatial:")
        return rc

    assert spatial() == 0
    assert spatial(lw=0) == INVAL and spatial(lh=0) == INVAL and spatial(lw=32768) == INVAL
    assert spatial(lw=24) == INVAL  # (24 * 3 bytes do not fit the left image's rows)
    for c in (0, 2, 5):
        assert spatial(lch=c) == INVAL and spatial(ch=c) == INVAL
    zero = w.copy()
    zero[1] = 0
    assert spatial(w=zero) == INVAL
    zero = h.copy()
    zero[0] = 0
    assert spatial(h=zero) == INVAL
    big = w.copy()
    big[0] = 32768
    assert spatial(w=big, stride=(big * 3).astype(np.uint32)) == INVAL
    assert spatial(stride=(w * 3 - 1).astype(np.uint32)) == INVAL
    assert spatial(bytes_=buf.size - 1) == INVAL  # the last pixel lies outside
    assert spatial(n=(1 << 20) + 1) == INVAL and spatial(res=None) == INVAL
    assert (res.view(np.uint32)[2::4] > 0).all()  # (the good call's records are still there)

    frames, win = clip(8, 1), clip(3, 9)
    lp, rp = pack_plain(frames), pack_plain(win)
    rec = np.zeros(16, np.uint8)

    def temporal(nl=8, nw=3, start=2, lch=3, rch=3, lw=lp[2], rh=rp[3], host=True):
        import torch

        L.cbh_clear_error()
        if host:
            rc = L.cbh_align_temporal(lp[0].ctypes.data, lp[0].size, nl, _ptr(lp[1]), _ptr(lw), _ptr(lp[3]), _ptr(lp[4]), lch,
                                      rp[0].ctypes.data, rp[0].size, nw, _ptr(rp[1]), _ptr(rp[2]), _ptr(rh), _ptr(rp[4]), rch,
                                      start, rec.ctypes.data, None, None, 0)
        else:
            d_l, d_r = torch.from_numpy(lp[0]).cuda(), torch.from_numpy(rp[0]).cuda()
            d_rec = torch.zeros(16, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            rc = L.cbh_align_temporal_dev(d_l.data_ptr(), nl, _ptr(lp[1]), _ptr(lw), _ptr(lp[3]), _ptr(lp[4]), lch,
                                          d_r.data_ptr(), nw, _ptr(rp[1]), _ptr(rp[2]), _ptr(rh), _ptr(rp[4]), rch, start,
                                          d_rec.data_ptr(), None, None, 0, None)
        if rc == INVAL:
            assert L.cbh_last_error().decode().startswith("align temporal:")
        return rc

    for host in (True, False):
        assert temporal(host=host) == 0
        assert temporal(nl=2, start=0, host=host) == INVAL  # W > nL
        assert temporal(nw=0, host=host) == INVAL
        assert temporal(start=6, host=host) == INVAL and temporal(start=-1, host=host) == INVAL  # P = 6
        assert temporal(start=5, host=host) == 0
        assert temporal(lch=2, host=host) == INVAL and temporal(rch=0, host=host) == INVAL
        zero = lp[2].copy()
        zero[7] = 0
        assert temporal(lw=zero, host=host) == INVAL
        zero = rp[3].copy()
        zero[0] = 0
        assert temporal(rh=zero, host=host) == INVAL
    assert temporal(nw=65) == INVAL and temporal(nl=65536) == INVAL

    import torch

    d_l, d_r = torch.from_numpy(np.ascontiguousarray(left)).cuda(), torch.from_numpy(buf).cuda()
    d_res = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def dev(lw=23, lch=3, ch=3, w=w, n=n, res=d_res.data_ptr()):
        return L.cbh_align_spatial_dev(d_l.data_ptr(), lw, 17, 69, lch, d_r.data_ptr(), n, _ptr(off), _ptr(w), _ptr(h),
                                       _ptr(st), ch, res, None, 0, None)

    assert dev() == 0
    assert dev(lw=0) == INVAL and dev(lch=2) == INVAL and dev(ch=5) == INVAL and dev(w=big) == INVAL
    assert dev(n=(1 << 20) + 1) == INVAL and dev(res=None) == INVAL


@pytest.mark.parametrize("entry", ["spatial_host", "spatial_dev", "temporal_host", "temporal_dev"])
def test_every_allocation_may_be_refused(lib, entry):
    """the walk of tests/test_error_paths.py: "fault_alloc_after" 0, 1, 2, ... until the call makes fewer allocations.
    Every refused call returns CBH_E_NOMEM, leaves no scratch handed out, and the next call gives the same results"""
    from cbird_amd import _lib

    L = lib
    left = R.textured(33, 21, 59)
    rights = [R.textured(17, 9, 61), R.textured(40, 31, 62)]
    frames, win = clip(6, 1), clip(2, 9)

    def call():
        if entry.startswith("spatial"):
            rc, res, tab = (spatial_host if entry == "spatial_host" else spatial_dev)(L, left, rights)
            return rc, res.tobytes() + tab.tobytes()
        rc, rec, means, cells = (temporal_host if entry == "temporal_host" else temporal_dev)(L, frames, win, 2)
        return rc, rec.tobytes() + means.tobytes() + cells.tobytes()

    rc, first = call()  # (one-time costs are not part of the walk)
    assert rc == 0
    refused = 0
    for k in range(100):
        live0, fired0 = _tuning(L, b"arena_live_bytes"), _tuning(L, b"fault_fired")
        L.cbh_set_tuning(b"fault_alloc_after", k)
        try:
            rc, _ = call()
        finally:
            L.cbh_set_tuning(b"fault_alloc_after", -1)
        if _tuning(L, b"fault_fired") == fired0:
            assert rc == 0
            break
        refused += 1
        assert rc == _lib.CBH_E_NOMEM, (k, rc)
        assert _tuning(L, b"arena_live_bytes") == live0, k
        rc, again = call()
        assert rc == 0 and again == first, k
    else:
        pytest.fail("the call never ran out of allocations to refuse")
    # the device entries take the image table and the planes from the arena (every optional output is given here); the
    # host entries stage two inputs, the record(s) and the table or the means and the cells in front of them
    assert refused == {"spatial_host": 6, "spatial_dev": 2, "temporal_host": 7, "temporal_dev": 2}[entry]


# ---- the Python entries -----------------------------------------------------------------------------------------------
def test_python_entries(lib):
    import torch

    from cbird_amd import align_spatial, align_temporal

    left = source(1, 4)
    rights = [source(k % 5, (1, 3, 4)[k % 3]) for k in range(7)]  # mixed channel counts: one call per count
    res, tab = align_spatial(left, rights, table=True)
    check_spatial("numpy", left, rights, res, tab.reshape(-1, 17, 17))
    assert tab.shape == (7, 17, 17)
    t_res = align_spatial(torch.from_numpy(left).cuda(), [torch.from_numpy(r).cuda() for r in rights])
    assert t_res.tobytes() == res.tobytes()
    t_res, t_tab = align_spatial(torch.from_numpy(left).cuda(), [torch.from_numpy(r).cuda() for r in rights], table=True)
    assert t_res.tobytes() == res.tobytes() and (t_tab == tab).all()
    assert len(align_spatial(left, [])) == 0
    name = "other sizes and channel counts"
    lf, rf, start = TCASES[name]
    wcells, wmeans, wrec = want_temporal(name)
    rec, means, cells = align_temporal(lf, rf, cells=True)  # start=None: 30 of 60
    assert start == 30 and (cells == wcells).all() and (means == wmeans).all()
    assert all(int(rec[f]) == wrec[f] for f in TFIELDS)
    rec2, means2 = align_temporal([torch.from_numpy(f).cuda() for f in lf], [torch.from_numpy(f).cuda() for f in rf], 30)
    assert rec2.tobytes() == rec.tobytes() and (means2 == means).all()
    with pytest.raises(ValueError):
        align_temporal(rf, lf)


def test_alignment_chains_into_difference_images(lib):
    """align_spatial -> alignment_transform -> difference_images on a planted shift: the pair is drawn through the
    transform and differs less than as it lies"""
    from cbird_amd import align_spatial, alignment_transform, difference_images

    left, right = A.planted(3, -5, seed=11)
    res = align_spatial(left, [right])
    assert (int(res[0]["min_x"]), int(res[0]["min_y"]), int(res[0]["min_sad"])) == (3, -5, 0)
    m = alignment_transform(res[0]["min_x"], res[0]["min_y"], left.shape, right.shape)
    _, det = difference_images(left, [right], m.reshape(1, 2, 3), pictures=False)
    _, apart = difference_images(left, [right], pictures=False)
    assert det[0]["warped"] == 1 and apart[0]["warped"] == 0
    assert det[0]["sum_total"] < apart[0]["sum_total"]
