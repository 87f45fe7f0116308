"""A plain NumPy model of cbh_idx64_clusters / cbh_idx64_cluster_labels (include/cbird_hip.h): the connected components
of a DctHashIndex's match graph.  Nodes: slots with id != 0 and hash != 0, in ascending id order.  Edges: nodes i != j
with popcount(h_i ^ h_j) < thresh.  np.bitwise_count on row blocks of the distinct hash values and a union-find over
their edges; nodes that share a hash value are joined when thresh >= 1 (their distance is 0).

Also here: the data shapes the device tests use, and what similar(mergeGroups=1) makes of a component, so that a test
can require from the model alone that its data shows where the two differ."""
import numpy as np

NO_NEIGHBOUR = 0xFF


def live_nodes(hashes, ids):
    """(ids, hashes) of the live slots in ascending id order; ValueError when two live slots hold one id"""
    h, i = np.asarray(hashes, np.uint64), np.asarray(ids, np.uint32)
    live = (i != 0) & (h != 0)
    h, i = h[live], i[live]
    order = np.argsort(i, kind="stable")
    h, i = h[order], i[order]
    if len(i) > 1 and (i[1:] == i[:-1]).any():
        raise ValueError("an id is held twice")
    return i, h


def _find(parent, x):
    root = x
    while parent[root] != root:
        root = parent[root]
    while parent[x] != root:
        parent[x], x = root, parent[x]
    return root


def cluster_labels(hashes, ids, thresh, block=512):
    """(ids, label = the smallest id of the node's component, nearest = distance to the nearest other node under
    thresh or 0xFF) per node in ascending id order"""
    nid, h = live_nodes(hashes, ids)
    n = len(nid)
    if n == 0:
        return nid, nid.copy(), np.zeros(0, np.uint8)
    uniq, inv, cnt = np.unique(h, return_inverse=True, return_counts=True)
    u = len(uniq)
    near_u = np.full(u, NO_NEIGHBOUR, np.int64)  # nearest OTHER value under thresh
    parent = list(range(u))
    for a in range(0, u, block):
        d = np.bitwise_count(uniq[a:a + block, None] ^ uniq[None, :]).astype(np.int64)
        d[np.arange(d.shape[0]), np.arange(a, a + d.shape[0])] = 99  # not its own neighbour
        edge = d < thresh
        near_u[a:a + block] = np.where(edge, d, NO_NEIGHBOUR).min(axis=1)
        rr, cc = np.nonzero(edge)
        below = cc < rr + a  # every edge once
        for r, c in zip((rr[below] + a).tolist(), cc[below].tolist()):
            ra, rb = _find(parent, r), _find(parent, c)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    root_u = np.array([_find(parent, x) for x in range(u)])
    shared = (cnt > 1) & (thresh >= 1)
    nearest = np.where(shared[inv], 0, near_u[inv])
    if thresh >= 1:
        comp = root_u[inv]  # equal hashes are one value: joined
    else:
        comp = np.arange(n)
    first = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(first, comp, np.arange(n))  # nodes are in id order: the first node has the smallest id
    return nid, nid[first[comp]], nearest.astype(np.uint8)


def clusters(hashes, ids, thresh, min_members=2):
    """the components with at least min_members nodes as lists of (id, score = nearest): members in ascending id,
    clusters in ascending first id"""
    nid, label, nearest = cluster_labels(hashes, ids, thresh)
    out = {}
    for i, l, s in zip(nid.tolist(), label.tolist(), nearest.tolist()):
        out.setdefault(l, []).append((i, s))
    return [g for _, g in sorted(out.items()) if len(g) >= min_members]


def brute_force(hashes, ids, thresh):
    """the definition, pair by pair in pure Python: {id: (label, nearest)}"""
    nid, h = live_nodes(hashes, ids)
    n = len(nid)
    adj = [[j for j in range(n) if j != i and bin(int(h[i]) ^ int(h[j])).count("1") < thresh] for i in range(n)]
    label, out = [-1] * n, {}
    for s in range(n):
        if label[s] < 0:
            stack, label[s] = [s], s
            while stack:
                for j in adj[stack.pop()]:
                    if label[j] < 0:
                        label[j] = s
                        stack.append(j)
    for i in range(n):
        near = min([bin(int(h[i]) ^ int(h[j])).count("1") for j in adj[i]], default=NO_NEIGHBOUR)
        out[int(nid[i])] = (int(nid[label[i]]), near)
    return out


# ---- data ---------------------------------------------------------------------------------------------------------------
def flip(h, bits):
    for b in bits:
        h ^= 1 << int(b)
    return h


def random_walks(n, seed, restart=0.2, max_flips=3):
    """n hashes: each is the one before with 0..max_flips random bits flipped, or (with probability `restart`) a fresh
    random value; then shuffled.  ids 1..n in the shuffled order"""
    rng = np.random.default_rng(seed)
    out, h = [], 0
    for k in range(n):
        if k == 0 or rng.random() < restart:
            h = int(rng.integers(1, 1 << 63))
        else:
            h = flip(h, rng.choice(64, int(rng.integers(0, max_flips + 1)), replace=False))
        out.append(h or 1)
    h = np.array(out, np.uint64)
    rng.shuffle(h)
    return h, np.arange(1, n + 1, dtype=np.uint32)


def chain(n, thresh, seed, descending=False):
    """a random-walk chain of thresh - 1 flipped bits per step; ids ascend (or descend) along it"""
    rng = np.random.default_rng(seed)
    h, out = int(rng.integers(1, 1 << 63)), []
    for _ in range(n):
        out.append(h)
        h = flip(h, rng.choice(64, thresh - 1, replace=False))
    ids = np.arange(1, n + 1, dtype=np.uint32)
    return np.array(out, np.uint64), ids[::-1].copy() if descending else ids


def hub(leaves, thresh, seed, hub_first=True):
    """a hub and `leaves` distinct hashes at distance 1..thresh - 1 from it (leaves mostly not adjacent to each other)"""
    rng = np.random.default_rng(seed)
    centre = int(rng.integers(1, 1 << 63))
    seen, out = {centre}, []
    while len(out) < leaves:
        x = flip(centre, rng.choice(64, int(rng.integers(1, thresh)), replace=False))
        if x not in seen:
            seen.add(x)
            out.append(x)
    h = np.array(([centre] + out) if hub_first else (out + [centre]), np.uint64)
    return h, np.arange(1, leaves + 2, dtype=np.uint32)


# ---- what -similar with mergeGroups makes of it ------------------------------------------------------------------------
def merge_route(hashes, ids, thresh, max_matches=5, min_matches=1):
    """similar(mergeGroups=1) on the host for these nodes (paths ordered like ids): searchIndex's per-needle lists --
    (score, id) order, filterSelf, cut at max_matches -- then filter_results with filterGroups and mergeGroupList.
    Groups as sorted id lists."""
    from cbird_amd import Media, SearchParams
    from cbird_amd.database import filter_results

    nid, h = live_nodes(hashes, ids)
    p = SearchParams(dctThresh=thresh, maxMatches=max_matches, minMatches=min_matches, mergeGroups=1)
    media = [Media(id=int(i), dctHash=int(x), path=f"{int(i):010d}") for i, x in zip(nid, h)]
    d = np.bitwise_count(h[:, None] ^ h[None, :]).astype(np.int64)
    results = []
    for k, m in enumerate(media):
        js = [j for j in np.nonzero(d[k] < thresh)[0].tolist() if j != k]
        js.sort(key=lambda j: (d[k, j], nid[j]))
        group = [m]
        for j in js[:max_matches]:
            group.append(Media(id=media[j].id, dctHash=media[j].dctHash, path=media[j].path, score=int(d[k, j])))
        results.append(group)
    return [sorted(x.id for x in g) for g in filter_results(p, results)]


def properties(hashes, ids, thresh, largest=400):
    """what a random set must hold to exercise the feature, from the model alone: (a cluster with two members at distance
    >= thresh, a singleton, a cluster that merge_route splits or repeats).  Components do not interact in
    mergeGroupList -- a group only ever absorbs groups that share a member with it -- so the third is decided per
    component, on components of at most `largest` nodes."""
    nid, h = live_nodes(hashes, ids)
    _, label, _ = cluster_labels(hashes, ids, thresh)
    comps = {}
    for k, l in enumerate(label.tolist()):
        comps.setdefault(l, []).append(k)
    singleton = any(len(c) == 1 for c in comps.values())
    far = split = False
    for c in comps.values():
        if len(c) < 3:
            continue
        hc = h[c]
        if not far and (np.bitwise_count(hc[:, None] ^ hc[None, :]) >= thresh).any():
            far = True
        if not split and len(c) <= largest:
            groups = merge_route(hc, nid[c], thresh)
            split = groups != [sorted(nid[c].tolist())]
        if far and split:
            break
    return far, singleton, split
