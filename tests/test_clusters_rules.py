"""CPU: tests/clusters_rules.py, the NumPy model of cbh_idx64_clusters, on hand-made cases and against the definition
pair by pair; and the defect of Media::mergeGroupList the clusters answer, on the issue's own chain."""
import numpy as np
import pytest

import clusters_rules as CR
from cbird_amd import Media
from cbird_amd.database import merge_group_list

A = 0x0123456789ABCDEF
C_ = CR.flip(A, [0, 1, 2])        # a ~ c: 3
B = CR.flip(C_, [10, 11, 12])     # c ~ b: 3, a !~ b: 6


def test_chain_is_one_cluster_of_three():
    h, ids = [A, B, C_], [1, 2, 3]  # path order a, b, c
    assert CR.clusters(h, ids, 5) == [[(1, 3), (2, 3), (3, 3)]]
    nid, label, near = CR.cluster_labels(h, ids, 5)
    assert nid.tolist() == [1, 2, 3] and label.tolist() == [1, 1, 1] and near.tolist() == [3, 3, 3]
    assert CR.clusters(h, ids, 3) == [] and CR.clusters(h, ids, 4, min_members=3) == [[(1, 3), (2, 3), (3, 3)]]


def test_merge_group_list_is_not_transitive_on_that_chain():
    """the groups of -similar in needle-path order are [a,c], [b,c], [c,a,b]: the merge leaves b and c in two groups"""
    a, b, c = (Media(id=i, path=p) for i, p in ((1, "a"), (2, "b"), (3, "c")))
    got = merge_group_list([[a, c], [b, c], [c, a, b]])
    assert [sorted(m.path for m in g) for g in got] == [["a", "b", "c"], ["b", "c"]]
    assert CR.merge_route([A, B, C_], [1, 2, 3], 5) != [[1, 2, 3]]
    assert CR.properties([A, B, C_, 0x7777], [1, 2, 3, 4], 5) == (True, True, True)


def test_id0_and_hash0_slots_stay_out():
    h, ids = [A, A, 0, A, CR.flip(A, [5])], [4, 0, 9, 2, 7]
    assert CR.cluster_labels(h, ids, 5)[0].tolist() == [2, 4, 7]
    assert CR.clusters(h, ids, 5) == [[(2, 0), (4, 0), (7, 1)]]
    # a hash-0 slot within reach of a node is no neighbour either
    assert CR.clusters([0b11, 0, 0xFF00], [1, 2, 3], 5) == []
    with pytest.raises(ValueError):
        CR.live_nodes([A, B], [3, 3])
    CR.live_nodes([A, 0], [3, 3])  # the second holder is not live


def test_min_members_two_and_three():
    far = 0xFFFF0000FFFF0000
    h, ids = [A, CR.flip(A, [1]), far, CR.flip(far, [2]), CR.flip(far, [3]), 0x5555], [1, 2, 3, 4, 5, 6]
    assert CR.clusters(h, ids, 5, 2) == [[(1, 1), (2, 1)], [(3, 1), (4, 1), (5, 1)]]
    assert CR.clusters(h, ids, 5, 3) == [[(3, 1), (4, 1), (5, 1)]]
    assert CR.clusters(h, ids, 5, 4) == []
    assert CR.cluster_labels(h, ids, 5)[2].tolist() == [1, 1, 1, 1, 1, CR.NO_NEIGHBOUR]


def test_thresholds_0_1_65():
    h, ids = [A, A, CR.flip(A, [9]), ~A & (2 ** 64 - 1)], [1, 2, 3, 4]
    assert CR.clusters(h, ids, 0) == []
    assert CR.cluster_labels(h, ids, 0)[1].tolist() == [1, 2, 3, 4]
    assert CR.cluster_labels(h, ids, 0)[2].tolist() == [CR.NO_NEIGHBOUR] * 4
    assert CR.clusters(h, ids, 1) == [[(1, 0), (2, 0)]]  # equal hashes only
    assert CR.clusters(h, ids, 63) == [[(1, 0), (2, 0), (3, 1)]]  # the complement is 63 away from id 3: not < 63 ...
    assert CR.clusters(h, ids, 64) == [[(1, 0), (2, 0), (3, 1), (4, 63)]]  # ... and joins at 64
    assert CR.clusters(h, ids, 65) == [[(1, 0), (2, 0), (3, 1), (4, 63)]]  # 65: every pair is an edge
    assert CR.clusters([A, ~A & (2 ** 64 - 1)], [1, 2], 64) == [] and CR.clusters([A, ~A & (2 ** 64 - 1)], [1, 2], 65) == [[(1, 64), (2, 64)]]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_a_permutation_of_the_slots_changes_nothing(seed):
    h, ids = CR.random_walks(300, seed)
    h[[5, 50]] = 0
    ids[[7, 70]] = 0
    want = CR.clusters(h, ids, 5)
    assert len(want) > 3
    perm = np.random.default_rng(seed).permutation(len(h))
    assert CR.clusters(h[perm], ids[perm], 5) == want
    got = CR.cluster_labels(h[perm], ids[perm], 5)
    assert all((a == b).all() for a, b in zip(got, CR.cluster_labels(h, ids, 5)))


@pytest.mark.parametrize("seed,thresh", [(4, 1), (5, 2), (6, 5), (7, 8), (8, 5)])
def test_model_equals_the_definition(seed, thresh):
    h, ids = CR.random_walks(150, seed, restart=0.15)
    if seed == 8:
        h[10:20] = h[10]  # a clique of equal hashes
    want = CR.brute_force(h, ids, thresh)
    nid, label, near = CR.cluster_labels(h, ids, thresh, block=64)
    assert {int(i): (int(l), int(s)) for i, l, s in zip(nid, label, near)} == want
    assert len(set(label.tolist())) < len(nid)


def test_shapes():
    h, ids = CR.chain(40, 5, 1)
    assert CR.clusters(h, ids, 5) == [[(i, 4) for i in range(1, 41)]]
    h, ids = CR.chain(40, 5, 1, descending=True)
    assert [i for i, _ in CR.clusters(h, ids, 5)[0]] == list(range(1, 41))
    for first in (True, False):
        h, ids = CR.hub(100, 5, 2, hub_first=first)
        (g,) = CR.clusters(h, ids, 5)
        assert len(g) == 101 and len(set(h.tolist())) == 101
