"""GPU: cbh_idx64_clusters / cbh_idx64_cluster_labels (cbird_amd/csrc/clusters.hip) -- the connected components of a
DctHashIndex's match graph -- against the NumPy model of tests/clusters_rules.py, exact equality everywhere.

The random sets are shuffled random walks of 0..3 flipped bits per step (seeds fixed below); every one with at least
63 entries must show, from the model alone, a cluster with two members at distance >= thresh (transitivity), a singleton,
and a cluster that similar(mergeGroups=1) would split or repeat.  Sets of one or two entries cannot hold the first."""
import ctypes as C

import numpy as np
import pytest

import clusters_rules as CR

THRESH = 5
SEEDS = {1: 1, 2: 1, 63: 1, 64: 1, 65: 1, 257: 1, 4097: 1}


@pytest.fixture(scope="module")
def lib(gpu):
    from cbird_amd import _lib

    return _lib.lib()


@pytest.fixture(autouse=True)
def knobs():
    """the chunking knobs at their defaults before and after every test"""
    from cbird_amd import _lib

    def reset():
        try:
            L = _lib.lib()
        except (OSError, FileNotFoundError):
            return
        L.cbh_set_tuning(b"cluster_chunk", 1 << 20)
        L.cbh_set_tuning(b"cluster_max_records", 1 << 26)

    reset()
    yield
    reset()


def _tuning(L, key):
    v = C.c_longlong(0)
    assert L.cbh_get_tuning(key, C.byref(v)) == 0
    return v.value


def index_of(gpu, h, ids, shards=None):
    idx = gpu.DctHashIndex(shards=shards)
    idx.load(np.asarray(h, np.uint64), np.asarray(ids, np.uint32))
    return idx


def agree(idx, h, ids, thresh=THRESH, min_members=(2,)):
    """labels, nearest and clusters of the index equal the model's on (h, ids); returns the clusters at min_members[0]"""
    want = CR.cluster_labels(h, ids, thresh)
    got = idx.cluster_labels(thresh)
    for g, w, name in zip(got, want, ("ids", "label", "nearest")):
        assert g.dtype == w.dtype and np.array_equal(g, w), name
    assert idx.last_cluster_stats.nodes == len(want[0])
    first = None
    for m in min_members:
        got_c, want_c = idx.clusters(thresh, m), CR.clusters(h, ids, thresh, m)
        assert got_c == want_c
        st = idx.last_cluster_stats
        assert (st.clusters, st.members) == (len(want_c), sum(len(g) for g in want_c))
        first = want_c if first is None else first
    return first


# ---- sizes --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_random_sets_at_the_sizes_where_kernels_go_wrong(gpu, n):
    h, ids = CR.random_walks(n, SEEDS[n])
    if n >= 63:
        assert CR.properties(h, ids, THRESH) == (True, True, True)
    agree(index_of(gpu, h, ids), h, ids, min_members=(2, 3))
    if n == 65:  # the ends of the threshold's range: no edges, equal hashes only, every pair
        idx = index_of(gpu, h, ids)
        assert agree(idx, h, ids, thresh=0) == [] and len(agree(idx, h, ids, thresh=65)) == 1
        agree(idx, h, ids, thresh=1)
        agree(idx, h, ids, thresh=64)
    if n == 2:  # the two as one cluster, and apart
        h[1] = CR.flip(int(h[0]), [3, 4])
        idx = index_of(gpu, h, ids)
        assert agree(idx, h, ids) == [[(1, 2), (2, 2)]] and agree(idx, h, ids, thresh=2) == []


@pytest.mark.gpu
def test_the_chain_merge_group_list_splits_is_one_cluster(gpu):
    a = 0x0123456789ABCDEF
    c = CR.flip(a, [0, 1, 2])
    b = CR.flip(c, [10, 11, 12])  # a ~ c, c ~ b, a !~ b; ids (= path order) a, b, c
    h, ids = np.array([a, b, c], np.uint64), np.array([1, 2, 3], np.uint32)
    assert CR.merge_route(h, ids, THRESH) == [[1, 2, 3], [2, 3]]
    idx = index_of(gpu, h, ids)
    assert agree(idx, h, ids, min_members=(2, 3)) == [[(1, 3), (2, 3), (3, 3)]]
    assert agree(idx, h, ids, thresh=3) == []


@pytest.mark.gpu
def test_five_chunks_flatten_between_them(gpu, lib):
    h, ids = CR.random_walks(4097, SEEDS[4097])
    assert CR.properties(h, ids, THRESH) == (True, True, True)
    idx = index_of(gpu, h, ids)
    assert lib.cbh_set_tuning(b"cluster_chunk", 1000) == 0 and _tuning(lib, b"cluster_chunk") == 1000
    whole = agree(idx, h, ids, min_members=(2, 3))
    assert idx.last_cluster_stats.chunks == 5 and idx.last_cluster_stats.rescans == 0
    assert len(whole) > 100
    lib.cbh_set_tuning(b"cluster_chunk", 1 << 20)
    assert idx.clusters(THRESH) == whole and idx.last_cluster_stats.chunks == 1
    for t in (0, 1, 8):
        agree(idx, h, ids, thresh=t)


# ---- shapes that stress the union ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("descending", [False, True])
def test_chain(gpu, lib, descending):
    """ids ascending along the chain: every hook finds a root; descending: every hook goes the wrong way (the retry)"""
    h, ids = CR.chain(3001, THRESH, 5, descending)
    idx = index_of(gpu, h, ids)
    (one,) = agree(idx, h, ids)
    assert len(one) == 3001
    lib.cbh_set_tuning(b"cluster_chunk", 700)
    assert idx.clusters(THRESH) == [one] and idx.last_cluster_stats.chunks == 5


@pytest.mark.gpu
@pytest.mark.parametrize("hub_first", [True, False])
def test_hub_with_4096_leaves(gpu, hub_first):
    h, ids = CR.hub(4096, THRESH, 6, hub_first)
    (one,) = agree(index_of(gpu, h, ids), h, ids)
    assert len(one) == 4097


@pytest.mark.gpu
def test_clique_of_2048_identical_hashes(gpu):
    """4.2 million records: the record block (set to 2^20 here) has to grow; everybody's nearest neighbour is 0 away"""
    h, ids = np.full(2048, 0x0F0F00FF12345678, np.uint64), np.arange(1, 2049, dtype=np.uint32)
    idx = index_of(gpu, h, ids)
    idx.set_record_capacity(1 << 20)
    (one,) = agree(idx, h, ids)
    assert one == [(i, 0) for i in range(1, 2049)]
    st = idx.last_cluster_stats
    assert st.records == 2048 * 2048 and st.chunks == 1 and st.rescans == 0


@pytest.mark.gpu
def test_clique_split_by_the_record_limit(gpu, lib):
    h, ids = np.full(2048, 0x0F0F00FF12345678, np.uint64), np.arange(1, 2049, dtype=np.uint32)
    idx = index_of(gpu, h, ids)
    idx.set_record_capacity(1 << 16)
    assert lib.cbh_set_tuning(b"cluster_max_records", 1 << 20) == 0
    agree(idx, h, ids)
    st = idx.last_cluster_stats
    assert st.rescans == 3 and st.chunks == 4 and st.records == 2048 * 2048  # 2048 -> 2 x 1024 -> 4 x 512 needles
    # one entry with more matches than the limit: nothing to halve
    lib.cbh_set_tuning(b"cluster_max_records", 1000)
    from cbird_amd import CbhError, _lib

    with pytest.raises(CbhError) as e:
        idx.clusters(THRESH)
    assert e.value.code == _lib.CBH_E_OVERFLOW
    lib.cbh_set_tuning(b"cluster_max_records", 1 << 26)
    assert len(idx.clusters(THRESH)[0]) == 2048


def two_cliques():
    """two cliques of distinct hashes (a centre and 20 one-bit neighbours, each held by 8 ids) whose only edge is x ~ y;
    returns (hashes, ids, id of x)"""
    a = 0x5A5A0000C3C3F00F
    b = CR.flip(a, range(40, 48))
    x, y = CR.flip(a, [40, 41]), CR.flip(b, [42, 43])
    left = [a] + [CR.flip(a, [k]) for k in range(20)]
    right = [b] + [CR.flip(b, [k]) for k in range(20, 40)]
    h = np.array((left + right) * 8 + [x, y], np.uint64)
    ids = np.random.default_rng(9).permutation(len(h)).astype(np.uint32) + 1
    return h, ids, int(ids[-2])


@pytest.mark.gpu
def test_two_cliques_joined_by_one_edge_and_index_states(gpu):
    h, ids, x = two_cliques()
    left = np.array(([True] * 21 + [False] * 21) * 8 + [True, False])
    d = np.bitwise_count(h[left][:, None] ^ h[~left][None, :])
    assert (int((d < THRESH).sum()), int(d[-1, -1])) == (1, 4)  # no edge between the sides but x ~ y
    idx = index_of(gpu, h, ids)
    (one,) = agree(idx, h, ids)
    assert len(one) == len(h)
    # remove(): the bridge goes, the cluster falls apart
    idx.remove([x])
    h2, ids2 = h.copy(), ids.copy()
    h2[-2], ids2[-2] = 0, 0
    apart = agree(idx, h2, ids2)
    assert [len(g) for g in apart] in ([168, 169], [169, 168])
    # add(): it joins again, in a new slot
    idx.add([gpu.Media(id=x, dctHash=int(h[-2]))])
    assert agree(idx, np.append(h2, h[-2]), np.append(ids2, np.uint32(x))) == [one]
    # slice(): the clusters of what the slice holds
    keep = np.sort(ids)[::3]
    sl = idx.slice(keep.tolist())
    mask = np.isin(ids, keep)
    agree(sl, h[mask], ids[mask], min_members=(2, 5))


@pytest.mark.gpu
def test_sharded_handle_equals_the_plain_one(gpu, lib):
    """cbh_idx64_create_sharded(1, 4): four logical shards on one device (no second device is involved)"""
    h, ids = CR.random_walks(4097, SEEDS[4097])
    h[[17, 3000]] = 0
    ids[[18, 3001]] = 0
    plain, sharded = index_of(gpu, h, ids), index_of(gpu, h, ids, shards=(1, 4))
    assert sharded.shard_count() == 4
    lib.cbh_set_tuning(b"cluster_chunk", 1000)
    want = agree(plain, h, ids)
    assert agree(sharded, h, ids) == want
    gone = [int(want[0][0][0]), int(want[3][1][0])]
    for idx in (plain, sharded):
        idx.remove(gone)
    h2, ids2 = h.copy(), ids.copy()
    h2[np.isin(ids, gone)], ids2[np.isin(ids, gone)] = 0, 0
    assert agree(sharded, h2, ids2) == agree(plain, h2, ids2)


# ---- protocol -----------------------------------------------------------------------------------------------------------
def raw_clusters(L, handle, thresh, min_members, cap_c, cap_m):
    first = np.full(cap_c + 1, 0xEE, np.uint64)
    members = np.full((max(cap_m, 1), 2), 0xEE, np.uint32)
    nc, nm = C.c_size_t(77), C.c_size_t(77)
    rc = L.cbh_idx64_clusters(handle, thresh, min_members, first.ctypes.data, cap_c, members.ctypes.data, cap_m, C.byref(nc),
                              C.byref(nm), None)
    return rc, nc.value, nm.value, first, members


@pytest.mark.gpu
def test_capacity_round_trip_and_bad_arguments(gpu, lib):
    from cbird_amd import _lib

    h, ids = CR.random_walks(257, SEEDS[257])
    idx = index_of(gpu, h, ids)
    want = CR.clusters(h, ids, THRESH)
    n_c, n_m = len(want), sum(len(g) for g in want)
    for cap_c, cap_m in ((0, 0), (n_c - 1, n_m), (n_c, n_m - 1)):
        rc, nc, nm, first, members = raw_clusters(lib, idx.handle, THRESH, 2, cap_c, cap_m)
        assert (rc, nc, nm) == (_lib.CBH_E_OVERFLOW, n_c, n_m)
        assert (first == 0xEE).all() and (members == 0xEE).all()  # nothing written
    rc, nc, nm, first, members = raw_clusters(lib, idx.handle, THRESH, 2, n_c, n_m)
    assert (rc, nc, nm) == (0, n_c, n_m) and int(first[n_c]) == n_m
    assert [[(int(members[t, 0]), int(members[t, 1])) for t in range(int(first[g]), int(first[g + 1]))]
            for g in range(n_c)] == want
    for thresh, mm in ((-1, 2), (66, 2), (THRESH, 1), (THRESH, 0)):
        assert raw_clusters(lib, idx.handle, thresh, mm, n_c, n_m)[0] == _lib.CBH_E_INVAL
    assert raw_clusters(lib, None, THRESH, 2, n_c, n_m)[0] == _lib.CBH_E_INVAL
    # labels: min(n, cap) entries written, *n_out = the node count
    n = C.c_size_t(0)
    a, b, c = np.zeros(300, np.uint32), np.zeros(300, np.uint32), np.full(300, 7, np.uint8)
    assert lib.cbh_idx64_cluster_labels(idx.handle, THRESH, a.ctypes.data, b.ctypes.data, c.ctypes.data, 100, C.byref(n),
                                        None) == 0
    wi, wl, wn = CR.cluster_labels(h, ids, THRESH)
    assert n.value == 257 and np.array_equal(a[:100], wi[:100]) and np.array_equal(b[:100], wl[:100])
    assert np.array_equal(c[:100], wn[:100]) and (c[100:] == 7).all() and not a[100:].any()
    assert lib.cbh_idx64_cluster_labels(idx.handle, THRESH, None, None, None, 0, C.byref(n), None) == 0 and n.value == 257
    assert lib.cbh_idx64_cluster_labels(idx.handle, 66, a.ctypes.data, b.ctypes.data, c.ctypes.data, 300, C.byref(n),
                                        None) == _lib.CBH_E_INVAL
    # an id held twice by live entries: not a DctHashIndex
    twice = ids.copy()
    twice[40] = twice[3]
    dup = index_of(gpu, h, twice)
    assert raw_clusters(lib, dup.handle, THRESH, 2, n_c, n_m)[0] == _lib.CBH_E_UNSUPPORTED
    dup.remove([int(twice[3])])  # both holders go: unique again
    h2, ids2 = h.copy(), twice.copy()
    h2[[3, 40]], ids2[[3, 40]] = 0, 0
    agree(dup, h2, ids2)
    # an empty and an unloaded-but-empty index
    assert index_of(gpu, [], []).clusters(THRESH) == []
    # the knobs refuse what they cannot take
    assert lib.cbh_set_tuning(b"cluster_chunk", 0) == lib.cbh_set_tuning(b"cluster_max_records", 0) == _lib.CBH_E_INVAL
    assert lib.cbh_set_tuning(b"cluster_chunk", (1 << 25) + 1) == _lib.CBH_E_INVAL
    assert _tuning(lib, b"cluster_chunk") == 1 << 20 and _tuning(lib, b"cluster_max_records") == 1 << 26


@pytest.mark.gpu
def test_a_refused_allocation_leaves_the_handle_usable(gpu, lib):
    from cbird_amd import CbhError, _lib

    h, ids = CR.random_walks(257, SEEDS[257])
    idx = index_of(gpu, h, ids)
    want = idx.clusters(THRESH)  # (also: the workspace and its record block exist now)
    live0, fired0 = _tuning(lib, b"arena_live_bytes"), _tuning(lib, b"fault_fired")
    lib.cbh_set_tuning(b"fault_alloc_after", 2)
    try:
        with pytest.raises(CbhError) as e:
            idx.clusters(THRESH)
    finally:
        lib.cbh_set_tuning(b"fault_alloc_after", -1)
    assert e.value.code == _lib.CBH_E_NOMEM and _tuning(lib, b"fault_fired") == fired0 + 1
    assert _tuning(lib, b"arena_live_bytes") == live0
    assert idx.clusters(THRESH) == want == CR.clusters(h, ids, THRESH)


@pytest.mark.gpu
def test_labels_into_device_arrays(gpu, lib):
    import torch

    h, ids = CR.random_walks(257, SEEDS[257])
    idx = index_of(gpu, h, ids)
    d_ids, d_label = (torch.zeros(257, dtype=torch.int32, device="cuda") for _ in range(2))
    d_near = torch.zeros(257, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n = C.c_size_t(0)
    assert lib.cbh_idx64_cluster_labels_dev(idx.handle, THRESH, d_ids.data_ptr(), d_label.data_ptr(), d_near.data_ptr(), 257,
                                            C.byref(n), None, None) == 0
    wi, wl, wn = CR.cluster_labels(h, ids, THRESH)
    assert n.value == 257
    assert np.array_equal(d_ids.cpu().numpy().view(np.uint32), wi) and np.array_equal(d_label.cpu().numpy().view(np.uint32), wl)
    assert np.array_equal(d_near.cpu().numpy(), wn)


# ---- the Python layer ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_database_clusters_orders_by_path(gpu):
    from cbird_amd import Media, SearchParams
    from cbird_amd.database import clusters

    h, ids = CR.random_walks(257, SEEDS[257])
    media = [Media(id=int(i), dctHash=int(x), path=f"/db/{1000 - int(i):04d}.jpg") for i, x in zip(ids, h)]  # paths descend
    idx = index_of(gpu, h, ids)
    for min_matches in (0, 1, 2):
        got = clusters(idx, media, SearchParams(dctThresh=THRESH, minMatches=min_matches))
        want = CR.clusters(h, ids, THRESH, max(2, min_matches + 1))
        want = sorted([sorted(g, reverse=True) for g in want], key=lambda g: -g[0][0])  # by path = by descending id
        assert [[(m.id, m.score) for m in g] for g in got] == want
    assert all(x.score == -1 for x in media)  # the haystack's own Media are untouched
    with pytest.raises(ValueError):
        clusters(idx, media, SearchParams(algo=SearchParams.AlgoColor))
