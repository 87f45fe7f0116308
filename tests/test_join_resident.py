"""The bucketed join's resident slot tables (cbird_amd/csrc/hamm64_join.hip, cbh_idx64_join_prepare / _release / _stats):
built once per join plan m = max(4, thresh), reused by every later joined call, dropped by every mutation -- and never a
different answer from the one the oracle gives on the handle's CURRENT contents.  Every test sets "scan_mfma" itself.
"""
import contextlib
import ctypes as C
import threading

import numpy as np
import pytest

K = 6


def _tuning(L, key):
    v = C.c_longlong(-2)
    assert L.cbh_get_tuning(key, C.byref(v)) == 0
    return int(v.value)


@contextlib.contextmanager
def _knobs(L, scan_mfma, **more):
    assert L.cbh_set_tuning(b"scan_mfma", scan_mfma) == 0
    for k, v in more.items():
        assert L.cbh_set_tuning(k.encode(), v) == 0
    try:
        yield
    finally:
        L.cbh_set_tuning(b"scan_mfma", 1)
        L.cbh_set_tuning(b"join_resident", 0)
        L.cbh_set_tuning(b"join_resident_mb", 2048)
        L.cbh_set_tuning(b"fault_alloc_after", -1)


def _reload(L, idx, h, ids):
    """cbh_idx64_load on a loaded handle reloads it (the Python wrapper keeps the reference's `if (!isLoaded())`)"""
    from cbird_amd import _lib

    h, ids = np.ascontiguousarray(h, np.uint64), np.ascontiguousarray(ids, np.uint32)
    _lib.check(L.cbh_idx64_load(idx.handle, h.ctypes.data, ids.ctypes.data, len(h)), "load")


def _check(idx, orc, h, ids, q, thresh, want=None, what=""):
    gi, gs, gc = idx.find_batch(q, thresh, K)
    wi, ws, wc = want if want is not None else orc.find64_batch(h, ids, q, thresh, K)
    assert (gc == wc).all() and (gi == wi).all() and (gs == ws).all(), (what, thresh)
    return gi, gc


def test_the_library_exports_the_join_entry_points_and_they_refuse_bad_arguments():
    from cbird_amd import _lib

    L = _lib.lib()
    for name in ("cbh_idx64_join_prepare", "cbh_idx64_join_release", "cbh_idx64_join_stats"):
        assert hasattr(L, name), name
    st = _lib.cbh_join_stats()
    assert L.cbh_idx64_join_stats(None, C.byref(st)) == _lib.CBH_E_INVAL
    assert L.cbh_idx64_join_prepare(None, 4) == _lib.CBH_E_INVAL
    assert L.cbh_idx64_join_release(None) == _lib.CBH_E_INVAL
    h = L.cbh_idx64_create(0)
    if h:  # (a handle needs a device)
        try:
            assert L.cbh_idx64_join_prepare(h, 0) == _lib.CBH_E_INVAL
            assert L.cbh_idx64_join_prepare(h, 9) == _lib.CBH_E_INVAL
            assert L.cbh_idx64_join_stats(h, None) == _lib.CBH_E_INVAL
            assert L.cbh_idx64_join_stats(h, C.byref(st)) == 0 and st.builds == 0 and st.bytes == 0 and st.plans == 0
        finally:
            L.cbh_idx64_destroy(h)


@pytest.mark.gpu
def test_every_plan_and_kernel_branch_equals_the_oracle_and_the_second_call_reuses_the_tables(gpu, orc):
    """40 000 slots x 12 000 needles; 1 100 slots and 4 100 needles share their low 16 bits, i.e. one value of chunk 0 in
    every plan: at plans 6..8 several jobs per value in both directions (512 slots / 2048 needles a job) and a needle tail
    that is no multiple of 8.  300 of those needles are planted slots with 0..3 of bits 16..63 flipped: the exact copies
    agree on every chunk, so a pair reported by two chunks would show in the counts."""
    from cbird_amd import _lib, synth

    L = _lib.lib()
    n, nq, low = 40_000, 12_000, np.uint64(0xBEE0)
    rng = np.random.default_rng(2024)
    h, ids = synth.make_hashes(n, seed=91, planted_frac=0.2)
    pos = rng.permutation(n)
    bucket, removed = pos[:1100], pos[1100:1100 + n // 50]
    h[bucket] = (h[bucket] & ~np.uint64(0xFFFF)) | low
    h[removed], ids[removed] = 0, 0
    q = h[rng.integers(0, n, nq)].copy()
    q[::3] ^= np.uint64(1) << rng.integers(1, 64, len(q[::3])).astype(np.uint64)
    qpos = rng.permutation(nq)
    qb, qnull = qpos[:4100], qpos[4100:4100 + nq // 100]
    q[qb] = (rng.integers(0, 2**48, 4100, dtype=np.uint64) << np.uint64(16)) | low
    near = h[bucket[:300]].copy()
    for i in range(300):
        for b in rng.choice(np.arange(16, 64), int(rng.integers(0, 4)), replace=False):
            near[i] ^= np.uint64(1) << np.uint64(b)
    q[qb[:300]] = near
    q[qnull] = 0
    in_bucket = (q & np.uint64(0xFFFF)) == low
    if int(in_bucket.sum()) % 8 == 0:  # (needles drawn from the slots add a few to the 4 100: keep the tail ragged)
        spare = np.flatnonzero(~in_bucket & (q != 0))[0]
        q[spare] = (q[spare] & ~np.uint64(0xFFFF)) | low
        in_bucket[spare] = True
    assert int(((h & np.uint64(0xFFFF)) == low).sum()) > 2 * 512
    assert int(in_bucket.sum()) > 2 * 2048 and int(in_bucket.sum()) % 8 != 0
    idx = gpu.DctHashIndex()
    idx.load(h, ids)
    with _knobs(L, 4):
        idx.join_prepare(4)
        assert idx.join_stats().builds == 1 and idx.join_stats().plans == 1 << 4
        for thresh in (1, 4, 5, 6, 7, 8):
            want = orc.find64_batch(h, ids, q, thresh, K)
            j0, s0 = _tuning(L, b"scan_joins"), idx.join_stats()
            _check(idx, orc, h, ids, q, thresh, want, "first call")
            s1 = idx.join_stats()
            assert _tuning(L, b"scan_joins") == j0 + 1
            assert s1.builds == s0.builds + (0 if thresh <= 4 else 1), thresh
            _check(idx, orc, h, ids, q, thresh, want, "second call")
            s2 = idx.join_stats()
            assert _tuning(L, b"scan_joins") == j0 + 2
            assert s2.hits > s1.hits and s2.builds == s1.builds, thresh
        st = idx.join_stats()
        assert st.plans == 0x1F0 and st.builds == 5 and st.failed_builds == 0
        assert st.bytes >= 12 * (4 + 5 + 6 + 7 + 8) * n
        idx.join_release()
        st = idx.join_stats()
        assert st.bytes == 0 and st.plans == 0 and st.drops == 5
        j0 = _tuning(L, b"scan_joins")  # released = not opted in: the per-call join, no tables
        _check(idx, orc, h, ids, q, 6, None, "after release")
        assert _tuning(L, b"scan_joins") == j0 + 1 and idx.join_stats().builds == 5


@pytest.mark.gpu
def test_a_stale_table_is_never_used(gpu, orc):
    """add, remove, load, load_device: each drops every plan, and the next finds (which rebuild them: the handle stays opted
    in) answer for the new contents -- a removed id never appears, an added entry does.  A slice starts without tables and
    leaves its parent's alone."""
    import torch

    from cbird_amd import _lib, synth

    L = _lib.lib()
    n = 20_000
    rng = np.random.default_rng(5)
    h, ids = synth.make_hashes(n, seed=17, planted_frac=0.2)
    extra, _ = synth.make_hashes(3000, seed=18, planted_frac=0.0)
    q = np.concatenate([h[rng.integers(0, n, 3000)], extra[:1000]])
    q[::4] ^= np.uint64(1) << rng.integers(1, 64, len(q[::4])).astype(np.uint64)
    q[7::97] = 0
    idx = gpu.DctHashIndex()
    idx.load(h, ids)
    with _knobs(L, 4):
        idx.join_prepare(8)
        idx.join_prepare(4)
        assert idx.join_stats().plans == (1 << 8) | (1 << 4)

        def settled(h_now, ids_now, before, what):
            st = idx.join_stats()
            assert st.plans == 0 and st.bytes == 0 and st.drops > before.drops, what
            out = [_check(idx, orc, h_now, ids_now, q, t, None, what) for t in (3, 8)]
            st2 = idx.join_stats()
            assert st2.builds > st.builds and st2.plans == (1 << 8) | (1 << 4), what
            return out

        before = idx.join_stats()
        add_ids = np.arange(n + 1, n + 3001, dtype=np.uint32)
        idx.add([gpu.Media(id=int(i), dctHash=int(x)) for i, x in zip(add_ids, extra)])
        h, ids = np.concatenate([h, extra]), np.concatenate([ids, add_ids])
        (gi3, gc3), _ = settled(h, ids, before, "add")
        assert np.isin(gi3[-1000:][gc3[-1000:] > 0], add_ids).any()  # (needles equal to added entries find them)

        before = idx.join_stats()
        rm = rng.choice(ids, 500, replace=False)
        idx.remove(rm.tolist())
        h, ids = h.copy(), ids.copy()
        gone = np.isin(ids, rm)
        h[gone], ids[gone] = 0, 0
        for gi, gc in settled(h, ids, before, "remove"):
            shown = gi[np.arange(K)[None, :] < np.minimum(gc, K)[:, None]]
            assert not np.isin(shown, rm).any()

        before = idx.join_stats()
        h, ids = synth.make_hashes(5000, seed=19, planted_frac=0.3)
        q[:2000] = h[rng.integers(0, 5000, 2000)]
        _reload(L, idx, h, ids)
        settled(h, ids, before, "load")

        before = idx.join_stats()
        h, ids = synth.make_hashes(7000, seed=20, planted_frac=0.3)
        dh, di = torch.from_numpy(h.view(np.int64)).cuda(), torch.from_numpy(ids.view(np.int32)).cuda()
        torch.cuda.synchronize()
        idx.load_device(dh.data_ptr(), di.data_ptr(), len(h))
        settled(h, ids, before, "load_device")

        keep = ids[::3]
        plans = idx.join_stats().plans
        part = idx.slice(keep.tolist())
        assert part.join_stats().builds == 0 and part.join_stats().plans == 0
        assert idx.join_stats().plans == plans != 0
        sel = np.isin(ids, keep)
        for t in (3, 8):
            _check(part, orc, h[sel], ids[sel], q, t, None, "slice")
            _check(idx, orc, h, ids, q, t, None, "parent of the slice")
        assert part.join_stats().builds == 0  # not opted in: the per-call join
        assert idx.join_stats().plans == plans


@pytest.mark.gpu
def test_remove_ids_only_drops_the_tables_of_a_features_index(gpu, orc):
    """DctFeaturesIndex::remove zeroes ids and keeps the hashes (ScanOpts::keep_id0), and its needles may be 0
    (ScanOpts::zero_needles): at dctThresh 5 before and after remove() the joined find_batch equals orc.fdct_find and the
    same calls on the matrix-core scan."""
    from cbird_amd import _lib, synth

    L = _lib.lib()
    m, k = 150, 100
    h, _ = synth.make_hashes(m * k, seed=23, planted_frac=0.4, max_dist=6)
    h[::501] = np.uint64(0x30)  # (within reach of a 0 needle)
    ids = np.repeat(np.arange(1, m + 1, dtype=np.uint32), k)
    needles = []
    for i in range(1, 41, 2):
        kp = h[ids == i].copy()
        kp[::9] ^= np.uint64(0x100)
        kp[3::25] = 0
        needles.append(gpu.Media(id=i, keyPointHashes=kp.tolist()))
    p = gpu.SearchParams(dctThresh=5)
    idx = gpu.DctFeaturesIndex()
    idx.load_flat(h, ids)

    def both(ids_now, what):
        out = {}
        for mode in (4, 2):
            L.cbh_set_tuning(b"scan_mfma", mode)
            out[mode] = [[(x.mediaId, x.score) for x in r] for r in idx.find_batch(needles, p)]
        assert out[4] == out[2], what
        for nd, got in zip(needles, out[4]):
            wi, ws = orc.fdct_find(h, ids_now, np.array(nd.keyPointHashes, np.uint64), nd.id, 5)
            assert got == list(zip(wi.tolist(), ws.tolist())), (what, nd.id)

    with _knobs(L, 4):
        idx.join_prepare(5)
        assert idx.join_stats().plans == 1 << 5
        both(ids, "before remove")
        assert idx.join_stats().hits >= 1
        d0 = idx.join_stats().drops
        idx.remove([5, 6, 21])
        assert idx.join_stats().plans == 0 and idx.join_stats().drops == d0 + 1
        ids_after = ids.copy()
        ids_after[np.isin(ids, [5, 6, 21])] = 0
        both(ids_after, "after remove")
        assert idx.join_stats().plans == 1 << 5


@pytest.mark.gpu
def test_sharded_handles_keep_tables_per_shard_and_prepare_the_needles_once(gpu, orc):
    """Five shards on one device: every shard has its own tables, `plans` does not wait for shards that hold nothing, and
    at thresholds 5 and 8 the needles' side is prepared ONCE per call ("join_needle_preps"), not once per shard; at
    threshold 2 the needles need no preparation at all."""
    from cbird_amd import _lib, synth

    L = _lib.lib()
    rng = np.random.default_rng(8)
    _lib.set_default_sharding((1, 5))
    try:
        with _knobs(L, 4):
            for n in (65_536, 100, 3):
                h, ids = synth.make_hashes(n, seed=31 + n, planted_frac=0.2)
                q = h[rng.integers(0, n, 3000)].copy()
                q[::3] ^= np.uint64(1) << rng.integers(1, 64, len(q[::3])).astype(np.uint64)
                q[11::50] = 0
                idx = gpu.DctHashIndex()
                assert idx.shard_count() == 5
                idx.load(h, ids)
                for t in (2, 5, 8):
                    idx.join_prepare(t)
                filled = sum(c > 0 for c in idx.shard_counts())
                st = idx.join_stats()
                assert st.plans == (1 << 4) | (1 << 5) | (1 << 8) and st.builds == 3 * filled, n
                for t, preps in ((2, 0), (5, 1), (8, 1)):
                    p0, j0 = _tuning(L, b"join_needle_preps"), _tuning(L, b"scan_joins")
                    _check(idx, orc, h, ids, q, t, None, n)
                    assert _tuning(L, b"join_needle_preps") == p0 + preps, (n, t)
                    assert _tuning(L, b"scan_joins") == j0 + filled, (n, t)
                assert idx.join_stats().builds == 3 * filled and idx.join_stats().hits >= 3 * filled
                extra, _ = synth.make_hashes(500, seed=77, planted_frac=0.0)
                extra[:100] = q[:100] | np.uint64(2)
                add_ids = np.arange(n + 1, n + 501, dtype=np.uint32)
                idx.add([gpu.Media(id=int(i), dctHash=int(x)) for i, x in zip(add_ids, extra)])
                assert idx.join_stats().plans == 0  # (the shard that took the batch lost its tables, the others kept theirs)
                assert idx.join_stats().bytes > 0 or filled == 1
                h2, ids2 = np.concatenate([h, extra]), np.concatenate([ids, add_ids])
                for t in (2, 5, 8):
                    _check(idx, orc, h2, ids2, q, t, None, ("after add", n))
    finally:
        _lib.set_default_sharding(None)


@pytest.mark.gpu
def test_concurrent_first_calls_build_each_plan_once(gpu, orc):
    from cbird_amd import _lib, synth

    L = _lib.lib()
    n = 30_000
    h, ids = synth.make_hashes(n, seed=41, planted_frac=0.2)
    q = h[::10].copy()
    q[::2] ^= np.uint64(0x4000)
    want = {t: orc.find64_batch(h, ids, q, t, K) for t in (4, 8)}
    with _knobs(L, 4, join_resident=1):
        idx = gpu.DctHashIndex()
        idx.load(h, ids)
        errors = []

        def work():
            try:
                for t in (4, 8):
                    _check(idx, orc, h, ids, q, t, want[t], "thread")
            except BaseException as e:  # noqa: BLE001 -- reported by the main thread
                errors.append(e)

        threads = [threading.Thread(target=work) for _ in range(8)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        st = idx.join_stats()
        assert st.builds == 2 and st.plans == (1 << 4) | (1 << 8) and st.failed_builds == 0


@pytest.mark.gpu
def test_allocation_failures_of_the_build_never_fail_or_falsify_a_search(gpu, orc):
    """The "fault_alloc_after" walk of tests/test_error_paths.py (k = 0, 1, 2, ... until no allocation is left to fail).
    Over join_prepare(8): every failing step is CBH_E_NOMEM and leaves no tables, no bytes, no arena block.  Over the first
    find_batch of an opted-in handle without tables: a step whose failure hit the BUILD (failed_builds grew) must succeed
    with the oracle's answer -- the call goes on per call; any other step succeeds with the oracle's answer or fails with a
    code that the same walk over a handle that is not opted in produces too (the two calls' allocation sequences differ, so
    the steps cannot be paired by number)."""
    from cbird_amd import _lib, synth

    L = _lib.lib()
    n = 20_000
    h, ids = synth.make_hashes(n, seed=43, planted_frac=0.2)
    q = h[::7].copy()
    q[::2] ^= np.uint64(0x8000)
    want = orc.find64_batch(h, ids, q, 8, K)

    def walk(step):
        for k in range(200):
            fired0 = _tuning(L, b"fault_fired")
            L.cbh_set_tuning(b"fault_alloc_after", k)
            try:
                step(k)
            finally:
                L.cbh_set_tuning(b"fault_alloc_after", -1)
            if _tuning(L, b"fault_fired") == fired0:
                return k
        pytest.fail("the call never ran out of allocations to fail")

    with _knobs(L, 4):
        idx = gpu.DctHashIndex()
        idx.load(h, ids)
        _check(idx, orc, h, ids, q, 8, want, "warm-up")  # (workspace and record block exist from here on)
        live0 = _tuning(L, b"arena_live_bytes")
        codes = []

        def prepare(k):
            fired0 = _tuning(L, b"fault_fired")
            rc = L.cbh_idx64_join_prepare(idx.handle, 8)
            if _tuning(L, b"fault_fired") != fired0:
                st = idx.join_stats()
                assert rc == _lib.CBH_E_NOMEM and st.bytes == 0 and st.plans == 0 and st.builds == 0, (k, rc)
                assert _tuning(L, b"arena_live_bytes") == live0, k
                codes.append(rc)
            else:
                assert rc == 0

        assert walk(prepare) >= 5 and len(codes) >= 5  # (four tables and the build's cursors)
        st = idx.join_stats()
        assert st.plans == 1 << 8 and st.builds == 1 and st.failed_builds == len(codes) and st.bytes >= 12 * 8 * n
        _check(idx, orc, h, ids, q, 8, want, "after the walk over join_prepare")
        idx.join_release()
        assert idx.join_stats().bytes == 0 and idx.join_stats().plans == 0

        plain = gpu.DctHashIndex()
        plain.load(h, ids)
        _check(plain, orc, h, ids, q, 8, want, "warm-up")
        plain_codes = set()

        def find_plain(k):
            try:
                _check(plain, orc, h, ids, q, 8, want, ("plain", k))
            except _lib.CbhError as e:
                plain_codes.add(e.code)

        walk(find_plain)
        assert plain.join_stats().builds == 0 and plain.join_stats().failed_builds == 0

        opted = gpu.DctHashIndex()
        opted.load([], [])
        opted.join_prepare(8)  # (nothing to build yet: opted in, no tables)
        _reload(L, opted, h, ids)  # (the storage exists from here on: the reloads below allocate nothing)
        _check(opted, orc, h, ids, q, 8, want, "warm-up")  # (and the workspace: every step meets the same allocations)
        assert opted.join_stats().builds == 1
        absorbed = []

        def find_opted(k):
            _reload(L, opted, h, ids)  # drops whatever the step before has built
            f0 = opted.join_stats().failed_builds
            assert opted.join_stats().plans == 0
            try:
                _check(opted, orc, h, ids, q, 8, want, ("opted", k))
            except _lib.CbhError as e:
                assert e.code in plain_codes and opted.join_stats().failed_builds == f0, (k, e)
            else:
                absorbed.append(opted.join_stats().failed_builds - f0)

        walk(find_opted)
        assert sum(absorbed) >= 5 and max(absorbed) == 1
        assert opted.join_stats().failed_builds == sum(absorbed)
        _check(opted, orc, h, ids, q, 8, want, "disarmed")
        assert opted.join_stats().plans == 1 << 8
        opted.join_release()
        assert opted.join_stats().bytes == 0
        assert _tuning(L, b"arena_live_bytes") == live0


@pytest.mark.gpu
def test_tables_over_the_budget_are_not_kept(gpu, orc):
    """"join_resident_mb" 1 against 9.6 MB of tables (100 000 slots, plan 8): the call prepares the slots itself"""
    from cbird_amd import _lib, synth

    L = _lib.lib()
    n = 100_000
    h, ids = synth.make_hashes(n, seed=47, planted_frac=0.2)
    q = h[::50].copy()
    q[::2] ^= np.uint64(0x20000)
    with _knobs(L, 4, join_resident=1, join_resident_mb=1):
        idx = gpu.DctHashIndex()
        idx.load(h, ids)
        j0 = _tuning(L, b"scan_joins")
        _check(idx, orc, h, ids, q, 8)
        st = idx.join_stats()
        assert _tuning(L, b"scan_joins") == j0 + 1
        assert st.bytes == 0 and st.builds == 0 and st.failed_builds >= 1 and st.plans == 0
        assert L.cbh_idx64_join_prepare(idx.handle, 8) == _lib.CBH_E_NOMEM
        L.cbh_set_tuning(b"join_resident_mb", 2048)
        idx.join_prepare(8)
        assert idx.join_stats().bytes >= 12 * 8 * n
        _check(idx, orc, h, ids, q, 8)
    assert _tuning(L, b"join_resident_mb") == 2048 and _tuning(L, b"join_resident") == 0


@pytest.mark.gpu
def test_the_cost_model_still_steps_aside_on_a_handle_with_tables(gpu):
    """The skewed set of test_bucketed_join_equals_the_scan_and_steps_aside_on_skewed_data (half of 400 000 slots share
    their low 16 bits) on a handle with plans 4 and 8 resident: at "scan_mfma" 3 the go / no-go estimate reads the cached
    FULL slot histogram, and still hands the calls to the scan."""
    import torch

    from cbird_amd import _lib, synth

    L = _lib.lib()
    n = 400_000
    rng = np.random.default_rng(77)
    skew, ids = synth.make_hashes(n, seed=4321, planted_frac=0.2)
    half = rng.permutation(n)[: n // 2]
    skew[half] = (skew[half] & ~np.uint64(0xFFFF)) | np.uint64(0x1234)
    ids[rng.integers(0, n, 500)] = 0
    q = skew.copy()
    q[rng.integers(0, n, 300)] = 0
    idx = gpu.DctHashIndex()
    idx.load(skew, ids)
    dq = torch.from_numpy(q.view(np.int64)).cuda()

    def run(dht):
        dout = torch.empty((n, K, 2), dtype=torch.int32, device="cuda")
        dcnt = torch.empty(n, dtype=torch.int32, device="cuda")
        tot = C.c_uint64(0)
        _lib.check(L.cbh_idx64_find_batch_dev(idx.handle, dq.data_ptr(), n, dht, K, dout.data_ptr(), dcnt.data_ptr(),
                                              C.byref(tot), None), "find_batch_dev")
        return int(tot.value), dcnt.cpu().numpy(), dout.cpu().numpy()

    with _knobs(L, 2):
        ref = {t: run(t) for t in (1, 4, 8)}
        idx.join_prepare(4)
        idx.join_prepare(8)
        assert idx.join_stats().plans == (1 << 4) | (1 << 8)
        L.cbh_set_tuning(b"scan_mfma", 3)
        j0 = _tuning(L, b"scan_joins")
        for t in (1, 4, 8):
            got = run(t)
            assert got[0] == ref[t][0] and (got[1] == ref[t][1]).all(), t
            m = np.arange(K)[None, :] < np.minimum(ref[t][1], K)[:, None]
            assert (got[2][m] == ref[t][2][m]).all(), t
        assert _tuning(L, b"scan_joins") - j0 < 3
        assert idx.join_stats().plans == (1 << 4) | (1 << 8)
