"""GPU suite for the grouped template match (cbird_amd/csrc/tmimages.hip, tmatch.hip): the descriptor match against a train
set per candidate, the ragged warp, and the chain cbh_template_match_pairs(_dev) held to the model of
tests/template_pairs_rules.py and, byte for byte, to cbh_template_match_images; then database.similar with
params.templateMatch.  Everything is compared bit for bit but the matrices m / tx (template_match_rules.m_tolerance)."""
import numpy as np
import pytest

import template_images_rules as M
import template_match_rules as R
import template_pairs_rules as P
from test_template_images import GUARD, _params, _tuning, check_chain, pack_ragged, spread

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(gpu):
    from cbird_amd import _lib, orb

    L = _lib.lib()
    orb.set_pattern(orb.synthetic_pattern())  # the model's (template_images_rules.oracles)
    L.cbh_set_tuning(b"orb_retain_order", 1)
    return L


# ---- 1. the match stage: a train set per candidate ----------------------------------------------------------------------
TRAIN_SETS = [1, 63, 1024, 1025, 2048]  # one row, just under a wave, at / past kTrainPiece and twice it


def _match_inputs(max_dist):
    """candidates of every train set's M.match_case in one launch, shuffled so that a set's candidates are not adjacent"""
    cases = [M.match_case(n_train, max_dist) for n_train in TRAIN_SETS]
    assert all(list(c[4][:len(M.QUERY_COUNTS)]) == M.QUERY_COUNTS for c in cases)
    cand = [(g, j) for g, c in enumerate(cases) for j in range(len(c[4]))]
    order = np.random.default_rng(17 + max_dist).permutation(len(cand))
    cand = [cand[k] for k in order]
    tmpl_first = np.concatenate([[0], np.cumsum(TRAIN_SETS)]).astype(np.uint64)
    tmpl_of = np.array([g for g, _ in cand], np.uint32)
    train = np.concatenate([c[0] for c in cases])
    train_xy = np.concatenate([c[1] for c in cases])
    desc = np.stack([cases[g][2][j] for g, j in cand])
    xy = np.stack([cases[g][3][j] for g, j in cand])
    counts = np.array([cases[g][4][j] for g, j in cand], np.uint32)
    recs, a, b, first = [], [], [], [0]
    for i, (g, j) in enumerate(cand):  # M.match_model, per candidate against its own set
        r = M.radius_match(cases[g][0], desc[i, :counts[i]], max_dist)
        ta, tb = M.gather(r, cases[g][1], xy[i])
        recs.append(r), a.append(ta), b.append(tb), first.append(first[-1] + len(r))
    model = (np.array(first, np.uint64), np.concatenate(recs), np.concatenate(a).astype(M.F32), np.concatenate(b).astype(M.F32))
    return (train, train_xy, tmpl_first, tmpl_of, desc, xy, counts), model


def _match_pairs_dev(L, inputs, max_dist, cap, records=True):
    import torch

    train, txy, tmpl_first, tmpl_of, desc, xy, counts = inputs
    n = len(counts)
    first = np.full(n + 1, 0xDEAD, np.uint64)
    d_train, d_txy, d_desc, d_xy, d_counts = (torch.from_numpy(np.ascontiguousarray(v)).cuda()
                                              for v in (train, txy, desc, xy, counts.view(np.int32)))
    mk = lambda elems, dt: torch.full((max(cap, 1) * elems + 16,), 7, dtype=dt, device="cuda")  # noqa: E731
    d_a, d_b, d_rec = mk(2, torch.float32), mk(2, torch.float32), mk(3, torch.int32)
    torch.cuda.synchronize()
    rc = L.cbh_tm_match_points_pairs_dev(d_train.data_ptr(), d_txy.data_ptr(), tmpl_first.ctypes.data, len(tmpl_first) - 1,
                                         tmpl_of.ctypes.data, d_desc.data_ptr(), d_xy.data_ptr(), d_counts.data_ptr(), n,
                                         M.KP_CAP, max_dist, d_rec.data_ptr() if records else None, d_a.data_ptr(),
                                         d_b.data_ptr(), cap, first.ctypes.data, 0, None)
    torch.cuda.synchronize()
    return rc, first, d_a.cpu().numpy(), d_b.cpu().numpy(), d_rec.cpu().numpy()


@pytest.mark.parametrize("max_dist", [0, 25, 256])
def test_match_stage_with_a_train_set_per_candidate(lib, max_dist):
    from cbird_amd import _lib

    inputs, (first, rec, a, b) = _match_inputs(max_dist)
    total = int(first[-1])
    per = np.diff(first.astype(np.int64))
    sizes = np.array(TRAIN_SETS)[inputs[3]]
    if max_dist == 256:
        assert (per == inputs[6].astype(np.int64) * sizes).all()  # every pair of the candidate's OWN set
    else:
        assert total >= 5 * 70
    rc, f, ga, gb, grec = _match_pairs_dev(lib, inputs, max_dist, total)
    assert rc == 0 and (f == first).all()
    assert (grec[:total * 3].reshape(-1, 3) == rec).all()
    assert ga[:total * 2].tobytes() == a.tobytes() and gb[:total * 2].tobytes() == b.tobytes()
    assert (ga[total * 2:] == 7).all() and (gb[total * 2:] == 7).all() and (grec[total * 3:] == 7).all()
    # one short: the count comes back complete and nothing is written
    rc, f, ga, gb, grec = _match_pairs_dev(lib, inputs, max_dist, total - 1, records=False)
    assert rc == _lib.CBH_E_OVERFLOW and (f == first).all()
    assert (ga == 7).all() and (gb == 7).all() and (grec == 7).all()


# ---- 2. the ragged warp --------------------------------------------------------------------------------------------------
PATCHES = [(1, 1), (3, 5), (5, 3), (7, 1), (131, 97), (160, 128)]  # four-pixel lanes cross rows and hit patch ends


def _warp_ragged(L, ch, stream=None):
    import torch

    rng = np.random.default_rng(60 + ch)
    imgs, ms = [], []
    for k, (tw, th) in enumerate(PATCHES):
        w, h = int(rng.integers(40, 200)), int(rng.integers(40, 200))
        img = rng.integers(1, 256, (h, w, ch), dtype=np.uint8)
        imgs.append(img[..., 0] if ch == 1 else img)
        ms.append(R.similarity(7.0 * k - 10, 0.8 + 0.15 * k, 3.5 + 2 * k, 1.25 * k))
    found = np.ones(len(PATCHES), np.uint8)
    found[2] = 0  # one candidate that came without a transform
    buf, off, w, h, st = pack_ragged(imgs, rng)
    sizes = [tw * th * ch for tw, th in PATCHES]
    poff, pos = [], 16  # 16-byte aligned patches with guard bytes in front of, between and behind them
    for s in sizes:
        poff.append(pos)
        pos += (s + 15) // 16 * 16 + 16
    poff = np.array(poff, np.uint64)
    tw = np.array([p[0] for p in PATCHES], np.uint32)
    th = np.array([p[1] for p in PATCHES], np.uint32)
    d_img = torch.from_numpy(buf).cuda()
    d_m = torch.from_numpy(np.stack(ms).astype(np.float64).reshape(-1)).cuda()
    d_f = torch.from_numpy(found).cuda()
    d_out = torch.full((pos,), GUARD, dtype=torch.uint8, device="cuda")
    d_ok = torch.full((len(PATCHES) + 16,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = L.cbh_warp_affine_ragged_dev(d_img.data_ptr(), len(PATCHES), off.ctypes.data, w.ctypes.data, h.ctypes.data,
                                      st.ctypes.data, ch, d_m.data_ptr(), d_f.data_ptr(), tw.ctypes.data, th.ctypes.data,
                                      poff.ctypes.data, d_out.data_ptr(), d_ok.data_ptr(), 0,
                                      stream.cuda_stream if stream else None)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    assert (d_img.cpu().numpy() == buf).all()
    return rc, d_out.cpu().numpy(), d_ok.cpu().numpy(), imgs, ms, found, poff, sizes


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_ragged_warp_equals_the_model_and_keeps_its_guards(lib, ch):
    import torch

    rc, out, ok, imgs, ms, found, poff, sizes = _warp_ragged(lib, ch)
    assert rc == 0
    keep = np.ones(len(out), bool)
    for i, ((tw, th), o, s) in enumerate(zip(PATCHES, poff, sizes)):
        keep[int(o): int(o) + s] = False
        got = out[int(o): int(o) + s]
        if not found[i]:
            assert ok[i] == 0 and not got.any(), i
            continue
        want, _ = R.warp_affine(imgs[i], ms[i], tw, th)
        assert want is not None and ok[i] == 1 and (got == want.reshape(-1)).all(), (i, tw, th)
    assert (out[keep] == GUARD).all() and (ok[len(PATCHES):] == GUARD).all()  # no lane wrote outside its own patch
    rc2, out2, ok2, *_ = _warp_ragged(lib, ch, torch.cuda.Stream())
    assert rc2 == 0 and (out2 == out).all() and (ok2 == ok).all()


# ---- 3. - 5. the chain ---------------------------------------------------------------------------------------------------
def _pairs_host(L, packed, ch, pt, pc, params=None):
    from cbird_amd.hashing import TEMPLATE_IMAGE_RESULT_DTYPE

    buf, off, w, h, st = packed
    p = _params() if params is None else params
    res = np.zeros(len(pt), TEMPLATE_IMAGE_RESULT_DTYPE)
    rc = L.cbh_template_match_pairs(buf.ctypes.data, buf.size, len(off), off.ctypes.data, w.ctypes.data, h.ctypes.data,
                                    st.ctypes.data, ch, pt.ctypes.data, pc.ctypes.data, len(pt), p.ctypes.data,
                                    res.ctypes.data, 0)
    return rc, res


def _pairs_dev(L, packed, ch, pt, pc, stream=None):
    import torch

    from cbird_amd.hashing import TEMPLATE_IMAGE_RESULT_DTYPE

    buf, off, w, h, st = packed
    p = _params()
    res = np.zeros(len(pt), TEMPLATE_IMAGE_RESULT_DTYPE)
    d_img = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    rc = L.cbh_template_match_pairs_dev(d_img.data_ptr(), len(off), off.ctypes.data, w.ctypes.data, h.ctypes.data,
                                        st.ctypes.data, ch, pt.ctypes.data, pc.ctypes.data, len(pt), p.ctypes.data,
                                        res.ctypes.data, 0, stream.cuda_stream if stream else None)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    assert (d_img.cpu().numpy() == buf).all()  # the source is not modified
    return rc, res


@pytest.fixture(scope="module")
def host_results(lib):
    """the host entry's records per channel count, computed once and never written to"""
    from cbird_amd.quality import pack_images

    out = {}
    for ch in (1, 3, 4):
        images, pt, pc, _ = P.pairs_fixture(ch)
        rc, res = _pairs_host(lib, pack_images(images), ch, pt, pc)
        assert rc == 0
        out[ch] = res
    return out


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_chain_equals_the_model(lib, host_results, ch):
    images, pt, pc, model = P.pairs_fixture(ch)
    assert P.pairs_conditions(images, pt, pc, model) == []
    tol, _ = R.m_tolerance()
    for p, want in enumerate(model):
        th, tw = images[pt[p]].shape[:2]
        check_chain(f"pair {p} {P.PAIRS[p]}", want, tol, host_results[ch][p], None, th, tw)
    assert not host_results[ch]["r"]["reserved"].any()


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_chain_equals_the_single_template_entry_byte_for_byte(lib, host_results, ch):
    from cbird_amd.hashing import template_match_images

    images, pt, pc, _ = P.pairs_fixture(ch)
    for t in sorted(set(pt.tolist())):
        ps = [p for p in range(len(pt)) if pt[p] == t]
        one = template_match_images(images[t], [images[pc[p]] for p in ps])
        for p, rec in zip(ps, one):
            assert rec.tobytes() == host_results[ch][p].tobytes(), (t, p)


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_order_streams_and_chunks(lib, host_results, ch):
    import torch

    from cbird_amd.hashing import template_match_pairs
    from cbird_amd.quality import pack_images

    images, pt, pc, _ = P.pairs_fixture(ch)
    want = host_results[ch]
    # a shuffled pair list gives the permuted records
    perm = np.random.default_rng(5).permutation(len(pt))
    rc, res = _pairs_host(lib, pack_images(images), ch, pt[perm].copy(), pc[perm].copy())
    assert rc == 0 and res.tobytes() == want[perm].tobytes()
    # the Python entry
    assert template_match_pairs(images, pt, pc).tobytes() == want.tobytes()
    # the device entry on a side stream, ragged rows and odd offsets
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    rc, res = _pairs_dev(lib, pack_ragged(images, np.random.default_rng(ch)), ch, pt, pc, side)
    assert rc == 0 and res.tobytes() == want.tobytes()
    # 1 MB chunks of a buffer that holds one image per MB: both entries cut the pairs into several chunks
    default = _tuning(lib, b"tmatch_chunk_mb")
    wide = spread(images)
    assert lib.cbh_set_tuning(b"tmatch_chunk_mb", 1) == 0
    try:
        rc, res5 = _pairs_host(lib, wide, ch, pt, pc)
        rc2, res6 = _pairs_dev(lib, wide, ch, pt, pc)
    finally:
        lib.cbh_set_tuning(b"tmatch_chunk_mb", int(default))
    assert rc == 0 and res5.tobytes() == want.tobytes()
    assert rc2 == 0 and res6.tobytes() == want.tobytes()


# ---- 6. arguments and refusals -------------------------------------------------------------------------------------------
def test_arguments(lib):
    from cbird_amd import _lib
    from cbird_amd.quality import pack_images

    INVAL = _lib.CBH_E_INVAL
    images, pt, pc, _ = P.pairs_fixture(3)
    buf, off, w, h, st = packed = pack_images(images)
    n = len(off)
    # zero pairs: nothing is read
    assert lib.cbh_template_match_pairs(None, 0, 0, None, None, None, None, 3, None, None, 0, None, None, 0) == 0
    assert lib.cbh_template_match_pairs_dev(None, 0, None, None, None, None, 3, None, None, 0, None, None, 0, None) == 0
    one = np.array([0], np.uint32)
    assert _pairs_host(lib, packed, 3, one, one)[0] == 0
    # an index equal to n_imgs, on either side
    bad = np.array([n], np.uint32)
    assert _pairs_host(lib, packed, 3, bad, one)[0] == INVAL and _pairs_host(lib, packed, 3, one, bad)[0] == INVAL
    # a bad channel count, bad params, an image that ends outside the buffer, a stride below the row
    assert _pairs_host(lib, packed, 2, one, one)[0] == INVAL and _pairs_host(lib, packed, 0, one, one)[0] == INVAL
    assert _pairs_host(lib, packed, 3, one, one, _params(cv_thresh=257))[0] == INVAL
    assert _pairs_host(lib, (buf[:-1], off, w, h, st), 3, one, one)[0] == INVAL
    assert _pairs_host(lib, (buf, off, w, h, (w * 3 - 1).astype(np.uint32)), 3, one, one)[0] == INVAL
    # null tables
    res = np.zeros(192, np.uint8)
    p = _params()
    tabs = (off.ctypes.data, w.ctypes.data, h.ctypes.data, st.ctypes.data)
    host = lambda tables=tabs, a=one.ctypes.data, b=one.ctypes.data, pp=p.ctypes.data, r=res.ctypes.data: (  # noqa: E731
        lib.cbh_template_match_pairs(buf.ctypes.data, buf.size, n, *tables, 3, a, b, 1, pp, r, 0))
    dev = lambda tables=tabs, a=one.ctypes.data, b=one.ctypes.data, img=16: (  # noqa: E731
        lib.cbh_template_match_pairs_dev(img, n, *tables, 3, a, b, 1, p.ctypes.data, res.ctypes.data, 0, None))
    assert host() == 0
    for k in range(4):
        assert host(tabs[:k] + (None,) + tabs[k + 1:]) == INVAL and dev(tabs[:k] + (None,) + tabs[k + 1:]) == INVAL
    assert host(a=None) == INVAL and host(b=None) == INVAL and host(pp=None) == INVAL and host(r=None) == INVAL
    assert dev(a=None) == INVAL and dev(b=None) == INVAL and dev(img=None) == INVAL
    # an image above ORB's limit: as a template, and as a candidate that reaches ORB unresized
    big = np.zeros((2, 8200, 3), np.uint8)
    small = np.zeros((40, 8200, 3), np.uint8)
    two = pack_images([big, small])
    assert _pairs_host(lib, two, 3, one, one)[0] == INVAL
    # (template 4100 wide, candidate 8200 wide and of a larger area: maxSize is 8200, so it reaches ORB as it is; the
    # single-template entry refuses the same call)
    wide_t = R.scene(np.random.default_rng(3), 80, 4100, 1)
    wide_c = np.full((41, 8200), 9, np.uint8)
    assert M.cand_target(4100, 80, 8200, 41, 200)[1:] == (8200, 41, False)
    assert _pairs_host(lib, pack_images([wide_t, wide_c]), 1, one, np.array([1], np.uint32))[0] == INVAL
    from test_template_images import _chain_host
    assert _chain_host(lib, wide_t, pack_images([wide_c]), patches=False)[0] == INVAL
    # the stage entries
    f2 = np.zeros(2, np.uint64)
    tf = np.array([0, 4], np.uint64)
    mp = lambda kp_cap=8, md=25, fi=f2, tfi=tf, of=one, g=1: lib.cbh_tm_match_points_pairs_dev(  # noqa: E731
        16, 16, None if tfi is None else tfi.ctypes.data, g, None if of is None else of.ctypes.data, 16, 16, 16, 1, kp_cap, md,
        None, 16, 16, 8, None if fi is None else fi.ctypes.data, 0, None)
    assert mp(0) == INVAL and mp(8, 257) == INVAL and mp(8, 25, None) == INVAL and mp(8, 25, f2, None) == INVAL
    assert mp(8, 25, f2, tf, None) == INVAL and mp(8, 25, f2, tf, np.array([1], np.uint32)) == INVAL
    assert mp(8, 25, f2, np.array([1, 4], np.uint64)) == INVAL and mp(8, 25, f2, np.array([0, 4, 2], np.uint64), one, 2) == INVAL
    assert lib.cbh_tm_match_points_pairs_dev(None, None, None, 0, None, None, None, None, 0, 8, 25, None, None, None, 0,
                                             f2.ctypes.data, 0, None) == 0
    o16, d8, s24 = np.array([16], np.uint64), np.array([8], np.uint32), np.array([24], np.uint32)
    wr = lambda c=3, dst=16, po=o16, tw=d8: lib.cbh_warp_affine_ragged_dev(  # noqa: E731
        16, 1, o16.ctypes.data, d8.ctypes.data, d8.ctypes.data, s24.ctypes.data, c, 16, 16,
        None if tw is None else tw.ctypes.data, d8.ctypes.data, None if po is None else po.ctypes.data, dst, None, 0, None)
    assert wr(2) == INVAL and wr(3, 17) == INVAL and wr(3, 16, np.array([8], np.uint64)) == INVAL and wr(3, 16, None) == INVAL
    assert wr(3, 16, o16, None) == INVAL and wr(3, 16, o16, np.array([0], np.uint32)) == INVAL
    assert lib.cbh_warp_affine_ragged_dev(None, 0, None, None, None, None, 3, None, None, None, None, None, None, None, 0,
                                          None) == 0


@pytest.mark.parametrize("entry", ["pairs", "pairs_dev", "match_points_pairs", "warp_ragged"])
def test_every_allocation_may_be_refused(lib, entry):
    """test_template_images' walk over each new entry: "fault_alloc_after" 0, 1, 2, ... until the call makes fewer
    allocations.  Every refused call returns CBH_E_NOMEM, leaves no scratch handed out, and the next call gives the same
    bytes"""
    from cbird_amd import _lib
    from cbird_amd.quality import pack_images

    L = lib
    images, pt, pc, _ = P.pairs_fixture(3)
    keep = [p for p in range(len(pt)) if pc[p] not in (P.ENLARGED, P.ENLARGED_2_2)][:8]  # (small images: the walk is long)
    pt, pc = pt[keep].copy(), pc[keep].copy()
    packed = pack_images(images)
    inputs, (first, *_rest) = _match_inputs(25) if entry == "match_points_pairs" else (None, (None,))

    def call():
        if entry == "pairs":
            rc, res = _pairs_host(L, packed, 3, pt, pc)
            return rc, res.tobytes()
        if entry == "pairs_dev":
            rc, res = _pairs_dev(L, packed, 3, pt, pc)
            return rc, res.tobytes()
        if entry == "warp_ragged":
            rc, out, ok, *_ = _warp_ragged(L, 3)
            return rc, out.tobytes() + ok.tobytes()
        rc, f, a, b, rec = _match_pairs_dev(L, inputs, 25, int(first[-1]))
        return rc, f.tobytes() + a.tobytes() + b.tobytes() + rec.tobytes()

    rc, first_result = call()  # (one-time costs are not part of the walk)
    assert rc == 0
    refused = 0
    for k in range(300):
        live0, fired0 = _tuning(L, b"arena_live_bytes"), _tuning(L, b"fault_fired")
        L.cbh_set_tuning(b"fault_alloc_after", k)
        try:
            rc, got = call()
        finally:
            L.cbh_set_tuning(b"fault_alloc_after", -1)
        if _tuning(L, b"fault_fired") == fired0:
            assert rc == 0
            break
        refused += 1
        assert rc == _lib.CBH_E_NOMEM, (k, rc)
        assert _tuning(L, b"arena_live_bytes") == live0, k
        rc, again = call()
        assert rc == 0 and again == first_result, k
    else:
        pytest.fail("the call never ran out of allocations to refuse")
    # (at least: the buffers the entry itself takes, before those of the stages it calls)
    assert refused >= {"pairs": 12, "pairs_dev": 11, "match_points_pairs": 6, "warp_ragged": 4}[entry]


# ---- 7. database.similar with params.templateMatch -----------------------------------------------------------------------
def test_similar_with_the_template_matcher_on_both_routes(lib):
    import oracle
    from cbird_amd import DctHashIndex, Media, SearchParams
    from cbird_amd.database import filter_results, search_index, similar
    from cbird_amd.templatematcher import TemplateMatcher

    images = [im for k, im in enumerate(P.pairs_images(3)) if k not in (P.FLAT, P.THIN)]
    images.append(np.ascontiguousarray(images[P.TMPL][::-1]))  # a dozen media
    orc = oracle.Oracle()
    media = []
    for k, im in enumerate(images):
        m = Media(id=k + 1, dctHash=int(orc.dcthash64(np.ascontiguousarray(M.gray(im)))), path=f"/img/{k:03d}.png")
        m.md5, m.image = f"{k:032x}", im
        media.append(m)
    assert len(media) == 12 and all(m.dctHash for m in media)
    # a loose threshold, chosen on the CPU: every needle has a candidate
    dist = [[bin(a.dctHash ^ b.dctHash).count("1") for b in media if b is not a] for a in media]
    p = SearchParams(dctThresh=max(min(d) for d in dist), templateMatch=True)
    idx = DctHashIndex()
    idx.load(np.array([m.dctHash for m in media], np.uint64), np.array([m.id for m in media], np.uint32))
    id_map = {m.id: m for m in media}
    flat = lambda groups: [[(m.id, m.score) for m in g] for g in groups]  # noqa: E731
    batched = similar(idx, media, p, batched=True, matcher=TemplateMatcher())
    loop = similar(idx, media, p, batched=False, matcher=TemplateMatcher())
    tm = TemplateMatcher()
    by_hand = filter_results(p, [[m] + tm.match(m, search_index(idx, m, p, id_map), p) for m in media])
    assert flat(batched) == flat(loop) == flat(by_hand)
    assert len(by_hand) >= 1 and any(len(g) > 1 for g in by_hand)
    # the matcher did remove results: without it the groups are larger
    plain = similar(idx, media, SearchParams(dctThresh=p.dctThresh), batched=True)
    assert sum(len(g) for g in plain) > sum(len(g) for g in batched)
    # matcher=None makes a TemplateMatcher of its own
    assert flat(similar(idx, media, p, batched=True)) == flat(batched)
