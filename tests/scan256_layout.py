"""Where a (row, needle) pair lands in the 256-bit scan kernels (cbird_amd/csrc/hamm256_mfma.hip, k_hamm256_scan in
hamm256_scan.hip), an exact-integer model of the three-field accumulator, a plain reference of the scan, and seeded fixtures
that put matches at chosen places of that layout.

Plain numpy, no GPU and nothing from cbird_amd.  The model restates route256 (hamm256_scan.hip), the launch arithmetic of
each kernel's launcher and the accumulator's bookkeeping; it never decides what the right answer is -- that is
reference_records(): every pair compared on all 256 bits.  It does not predict what the hardware rounds; it proves that a
fixture reaches the state it names.

Bit i of a descriptor is bit (i & 7) of byte i >> 3, i.e. bit (i & 31) of the little-endian 32-bit word i >> 5.  The
matrix-core kernels put words 2k + half of chunk k on the K axis (K block = one word = 32 bits): the first MFMA of a needle
tile covers bits 0..63, the second bits 64..127; the prefilter kernels stop there.

Layout:
  * MFMA C/D: lane L holds needle column r = L & 31, half = L >> 5; register g (0..15) of a row tile is the tile's row
    (g & 3) + 8 (g >> 2) + 4 half;
  * k_hamm256_mfma3<12,2>: wave W = 4 wg + w owns row tiles 12 W .. 12 W + 11 (1536 rows per workgroup), groups of 2;
    triple p = needle tiles 3p, 3p+1, 3p+2 as fields 0, 1, 2 of one accumulator; blockIdx.y = p // tpc3;
  * k_hamm256_mfma<6,3,KCH>: 6 tiles per wave (768 rows per workgroup), groups of 3, one needle tile per accumulator,
    blockIdx.y = tile // tpc, two tiles per trip of the needle loop and a tail step for an odd count;
  * k_hamm256_small<NT>: grid min(2048, ceil(row tiles / 4)); wave w of workgroup b walks row tiles
    4 b + w + stride (4 trip + u), stride = 4 grid, u = 0..3 the prefetch slot; needle tile q is field q % 3 of
    accumulator q // 3, tiles >= NT do not exist (their field stays at its start value);
  * k_hamm256_scan<8,4>: 2048 rows per workgroup, thread t keeps rows t + 256 j (j = 0..7); needles in chunks of q_chunk
    (blockIdx.y), blocks of 4 inside a chunk, the last block repeating its last needle.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

K_SCAN, K_MFMA2, K_MFMA4, K_MFMA3, K_SMALL4, K_SMALL8, K_SMALL16 = (1 << i for i in range(7))
KERNEL_NAMES = {K_SCAN: "k_hamm256_scan", K_MFMA2: "k_hamm256_mfma<6,3,2>", K_MFMA4: "k_hamm256_mfma<6,3,4>",
                K_MFMA3: "k_hamm256_mfma3", K_SMALL4: "k_hamm256_small<4>", K_SMALL8: "k_hamm256_small<8>",
                K_SMALL16: "k_hamm256_small<16>"}
PATHS = ("mfma", "mfma_rows", "valu")  # the values of conftest's scan256_path
PRE128_MAX_THRESH = 40  # kPre128MaxThresh
SHARD_RUN = 16384  # Shards256::kShardRun
TWO24 = 1 << 24


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


# ---- bits -------------------------------------------------------------------------------------------------------------
def rand_rows(rng, n: int) -> np.ndarray:
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def to_bits(rows) -> np.ndarray:
    return np.unpackbits(np.asarray(rows, np.uint8), axis=-1, bitorder="little")


def from_bits(bits) -> np.ndarray:
    return np.packbits(np.asarray(bits, np.uint8), axis=-1, bitorder="little")


def flipped(desc, positions) -> np.ndarray:
    b = to_bits(desc).copy()
    b[np.asarray(list(positions), np.int64)] ^= 1
    return from_bits(b)


def flip_in(rng, desc, k: int, lo: int, hi: int) -> np.ndarray:
    """`desc` with k random bits of [lo, hi) flipped"""
    return flipped(desc, lo + rng.choice(hi - lo, int(k), replace=False))


def word_dist(a, b) -> np.ndarray:
    """per 32-bit word Hamming distances, [..., 8]"""
    a = np.ascontiguousarray(a, np.uint8).view(np.uint32)
    b = np.ascontiguousarray(b, np.uint8).view(np.uint32)
    return np.bitwise_count(a ^ b).astype(np.int64)


def dist(a, b) -> np.ndarray:
    return word_dist(a, b).sum(-1)


def dist128(a, b) -> np.ndarray:
    return word_dist(a, b)[..., :4].sum(-1)


# ---- placement --------------------------------------------------------------------------------------------------------
def reg_row(g, half):
    """row (in its tile) of accumulator register g of a lane in `half`"""
    return (g & 3) + 8 * (g >> 2) + 4 * half


def row_reg(rit):
    """inverse of reg_row: (g, half) of row rit of a tile"""
    rit = np.asarray(rit)
    return (rit & 3) + 4 * (rit >> 3), (rit >> 2) & 1


def route(n: int, nq: int, thresh: int, path: str, forced: bool = True) -> int:
    """the kernel route256 (hamm256_scan.hip) picks: path as conftest's scan256_path ("mfma" = "scan256_mfma" 2 + "scan256_small" 1,
    "mfma_rows" = 2 + 0, "valu" = 0); forced=False is "scan256_mfma" 1, the shipped default"""
    if path == "valu" or thresh < 1 or thresh > 257:
        return K_SCAN
    if not forced and not (nq >= 64 and n >= 4096):
        return K_SCAN
    n_tiles = _cdiv(nq, 32)
    if path == "mfma" and thresh <= PRE128_MAX_THRESH and n_tiles <= 16 and (n >= 4096 or forced) and n <= (1 << 27) - 64:
        return K_SMALL4 if n_tiles <= 4 else K_SMALL8 if n_tiles <= 8 else K_SMALL16
    if thresh <= PRE128_MAX_THRESH and n_tiles >= 3:
        return K_MFMA3
    return K_MFMA2 if thresh <= PRE128_MAX_THRESH else K_MFMA4


def launch_mfma3(n: int, nq: int) -> dict:
    n_tiles = _cdiv(nq, 32)
    n_triples = _cdiv(n_tiles, 3)
    wgs = _cdiv(n, 1536)
    tpc = 43
    while tpc > 2 and wgs * _cdiv(n_triples, tpc) < 8192:
        tpc = (tpc + 1) >> 1
    chunks = _cdiv(n_triples, tpc)
    if chunks > 65535:
        tpc = (n_triples + 65534) // 65535
        chunks = _cdiv(n_triples, tpc)
    return dict(n_tiles=n_tiles, n_triples=n_triples, wgs=wgs, tpc=tpc, chunks=chunks, pad_tiles=3 * n_triples - n_tiles)


def launch_mfma(n: int, nq: int) -> dict:
    n_tiles = _cdiv(nq, 32)
    wgs = _cdiv(n, 768)
    tpc = 128
    while tpc > 4 and wgs * _cdiv(n_tiles, tpc) < 8192:
        tpc >>= 1
    chunks = _cdiv(n_tiles, tpc)
    if chunks > 65535:
        tpc = (n_tiles + 65534) // 65535
        chunks = _cdiv(n_tiles, tpc)
    return dict(n_tiles=n_tiles, wgs=wgs, tpc=tpc, chunks=chunks, last_chunk_tiles=n_tiles - (chunks - 1) * tpc)


def launch_small(n: int, nq: int) -> dict:
    n_tiles = _cdiv(nq, 32)
    assert n_tiles <= 16
    nt = 4 if n_tiles <= 4 else 8 if n_tiles <= 8 else 16
    row_tiles = _cdiv(n, 32)
    grid = min(2048, _cdiv(row_tiles, 4))
    return dict(n_tiles=n_tiles, nt=nt, na=(nt + 2) // 3, group=3 if ((nt + 2) // 3) % 3 == 0 else 2, row_tiles=row_tiles,
                grid=grid, stride=4 * grid)


def launch_scan(n: int, nq: int) -> dict:
    tiles = _cdiv(n, 2048)
    q_chunk = 4096
    while q_chunk > 256 and tiles * _cdiv(nq, q_chunk) < 8192:
        q_chunk >>= 1
    chunks = _cdiv(nq, q_chunk)
    if chunks > 65535:
        q_chunk = _cdiv(_cdiv(nq, 65535), 4) * 4
        chunks = _cdiv(nq, q_chunk)
    return dict(tiles=tiles, q_chunk=q_chunk, chunks=chunks, last_chunk=nq - (chunks - 1) * q_chunk)


def _row_part(row):
    row = np.asarray(row, np.int64)
    g, half = row_reg(row & 31)
    return row >> 5, g, half


def place_mfma3(row, needle, n: int, nq: int) -> dict:
    L = launch_mfma3(n, nq)
    tile, g, half = _row_part(row)
    needle = np.asarray(needle, np.int64)
    qt = needle >> 5
    w = tile // 12
    return dict(wg=w >> 2, wave=w & 3, tile=tile % 12, group=(tile % 12) // 2, g=g, half=half, r=needle & 31,
                field=qt % 3, triple=qt // 3, chunk=(qt // 3) // L["tpc"])


def place_mfma(row, needle, n: int, nq: int) -> dict:
    L = launch_mfma(n, nq)
    tile, g, half = _row_part(row)
    needle = np.asarray(needle, np.int64)
    qt = needle >> 5
    chunk = qt // L["tpc"]
    q0 = chunk * L["tpc"]
    q1 = np.minimum(L["n_tiles"], q0 + L["tpc"])
    w = tile // 6
    return dict(wg=w >> 2, wave=w & 3, tile=tile % 6, group=(tile % 6) // 3, g=g, half=half, r=needle & 31, chunk=chunk,
                tail=((q1 - q0) % 2 == 1) & (qt == q1 - 1), second=((qt - q0) % 2 == 1))


def place_small(row, needle, n: int, nq: int) -> dict:
    L = launch_small(n, nq)
    tile, g, half = _row_part(row)
    needle = np.asarray(needle, np.int64)
    qt = needle >> 5
    w, k = tile % L["stride"], tile // L["stride"]
    return dict(wg=w >> 2, wave=w & 3, u=k & 3, trip=k >> 2, g=g, half=half, r=needle & 31, field=qt % 3, acc=qt // 3,
                group=(qt // 3) // L["group"], last_tile=tile == L["row_tiles"] - 1)


def place_scan(row, needle, n: int, nq: int) -> dict:
    L = launch_scan(n, nq)
    row, needle = np.asarray(row, np.int64), np.asarray(needle, np.int64)
    chunk = needle // L["q_chunk"]
    q0 = chunk * L["q_chunk"]
    q1 = np.minimum(nq, q0 + L["q_chunk"])
    qb = q0 + (needle - q0) // 4 * 4
    return dict(wg=row // 2048, slot=(row % 2048) // 256, thread=row % 256, chunk=chunk, block=(needle - q0) // 4,
                pos=(needle - q0) % 4, ragged_block=qb + 4 > q1)


# ---- the three-field accumulator, in exact integers ----------------------------------------------------------------------
@dataclasses.dataclass
class AccStates:
    fields: np.ndarray  # [..., 3] the final 8-bit fields 128 + b - d_f (a field without a tile: 64 + b)
    end_ge: np.ndarray  # the end value is >= 2^24 (the kernel's `moved`)
    mfma_ge: np.ndarray  # the value after one of the first five MFMAs is
    block_ge: np.ndarray  # the value after the first K block of some MFMA is
    partials: np.ndarray  # [..., 12] the value after every K block


def accumulator_model(row, needles3, thresh: int, active=(True, True, True)) -> AccStates:
    """row [..., 32] against the three needles [..., 3, 32] that share its accumulator: C0 = 2^23 + (64 + b) 65793, and
    K block k (bits 32 k .. 32 k + 31, k = 0..3) of field f adds (16 - d_block) 2^(8 f); fields in order 0, 1, 2"""
    b = thresh - 1
    assert 0 <= b <= 127
    row = np.asarray(row, np.uint8)
    needles3 = np.asarray(needles3, np.uint8)
    d = word_dist(row[..., None, :], needles3)[..., :4]  # [..., 3, 4]
    val = np.full(d.shape[:-2], (1 << 23) + (64 + b) * 65793, np.int64)
    parts = []
    for f in range(3):
        for k in range(4):
            if active[f]:
                val = val + (16 - d[..., f, k]) * (1 << (8 * f))
            parts.append(val)
    parts = np.stack(parts, -1)
    low = parts[..., -1] - (1 << 23)
    fields = np.stack([(low >> (8 * f)) & 0xFF for f in range(3)], -1)
    want = np.stack([np.where(active[f], 128 + b - d[..., f, :].sum(-1), 64 + b) for f in range(3)], -1)
    assert np.array_equal(fields, want), "a field borrowed or carried"
    return AccStates(fields, parts[..., 11] >= TWO24, (parts[..., [1, 3, 5, 7, 9]] >= TWO24).any(-1),
                     (parts[..., 0::2] >= TWO24).any(-1), parts)


def register_needles(needles, triple: int, col, nq=None) -> np.ndarray:
    """the three needles of column `col` of triple `triple` [..., 3, 32]; zero descriptors past nq (the padding)"""
    needles = np.asarray(needles, np.uint8)
    nq = len(needles) if nq is None else nq
    col = np.asarray(col, np.int64)
    out = np.zeros(col.shape + (3, 32), np.uint8)
    for f in range(3):
        j = (3 * triple + f) * 32 + col
        ok = j < nq
        out[..., f, :] = np.where(ok[..., None], needles[np.minimum(j, nq - 1)], 0)
    return out


# ---- reference ----------------------------------------------------------------------------------------------------------
def reference_records(rows, needles, thresh: int) -> np.ndarray:
    """every pair with popcount(row ^ needle) < thresh as sorted records needle << 41 | dist << 32 | row (plain popcounts)"""
    r = np.ascontiguousarray(rows, np.uint8).reshape(-1, 32).view(np.uint64)
    q = np.ascontiguousarray(needles, np.uint8).reshape(-1, 32).view(np.uint64)
    out = []
    block = max(1, (1 << 22) // max(1, len(r)))
    for j0 in range(0, len(q), block):
        qb = q[j0:j0 + block]
        d = np.zeros((len(qb), len(r)), np.uint16)
        for w in range(4):
            d += np.bitwise_count(qb[:, None, w] ^ r[None, :, w])
        j, i = np.nonzero(d < thresh)
        out.append(((j + j0).astype(np.uint64) << np.uint64(41)) | (d[j, i].astype(np.uint64) << np.uint64(32))
                   | i.astype(np.uint64))
    return np.sort(np.concatenate(out)) if out else np.zeros(0, np.uint64)


def reference_records_matmul(rows, needles, thresh: int, chunk: int = 0) -> np.ndarray:
    """the same records from a +-1 float32 matrix product: dot = 256 - 2 dist, exact since |dot| <= 256"""
    rows = np.asarray(rows, np.uint8).reshape(-1, 32)
    chunk = chunk or max(1024, (1 << 25) // max(1, len(needles)))  # (128 MB of products at a time)
    qs = np.ascontiguousarray((1.0 - 2.0 * to_bits(np.asarray(needles, np.uint8).reshape(-1, 32)).astype(np.float32)).T)
    out = []
    for i0 in range(0, len(rows), chunk):
        rs = 1.0 - 2.0 * to_bits(rows[i0:i0 + chunk]).astype(np.float32)
        dot = rs @ qs
        i, j = np.nonzero(dot > 256 - 2 * thresh)
        d = ((256.0 - dot[i, j]) * 0.5).astype(np.uint64)
        out.append((j.astype(np.uint64) << np.uint64(41)) | (d << np.uint64(32)) | (i + i0).astype(np.uint64))
    return np.sort(np.concatenate(out)) if out else np.zeros(0, np.uint64)


def reference(rows, needles, thresh: int) -> np.ndarray:
    """the popcount form for small cases, the matrix product for large ones (tested against each other)"""
    if len(rows) * len(needles) > (1 << 24):
        return reference_records_matmul(rows, needles, thresh)
    return reference_records(rows, needles, thresh)


def pack_records(q, d, row) -> np.ndarray:
    return ((np.asarray(q).astype(np.uint64) << np.uint64(41)) | (np.asarray(d).astype(np.uint64) << np.uint64(32))
            | np.asarray(row).astype(np.uint64))


def unpack(rec) -> np.ndarray:
    """records -> rows (needle, dist, row)"""
    r = np.asarray(rec, np.uint64)
    return np.stack([(r >> np.uint64(41)).astype(np.int64), ((r >> np.uint64(32)) & np.uint64(0x1FF)).astype(np.int64),
                     (r & np.uint64(0xFFFFFFFF)).astype(np.int64)], axis=1)


def restrict(rec, q0: int, q1: int) -> np.ndarray:
    """the records of needles [q0, q1), renumbered from 0 (sorted stays sorted)"""
    r = np.asarray(rec, np.uint64)
    q = r >> np.uint64(41)
    keep = (q >= q0) & (q < q1)
    return r[keep] - (np.uint64(q0) << np.uint64(41))


def below(rec, thresh: int) -> np.ndarray:
    """the records of a lower threshold out of a sorted list (order is kept: (needle, dist, row))"""
    r = np.asarray(rec, np.uint64)
    return r[((r >> np.uint64(32)) & np.uint64(0x1FF)) < thresh]


def multiset_diff(got, want):
    """(missing, extra): records of `want` not in `got` and the other way round, as multisets"""
    g, w = np.sort(np.asarray(got, np.uint64)), np.sort(np.asarray(want, np.uint64))
    gv, gc = np.unique(g, return_counts=True)
    wv, wc = np.unique(w, return_counts=True)
    allv = np.union1d(gv, wv)
    gn = np.zeros(len(allv), np.int64)
    wn = np.zeros(len(allv), np.int64)
    gn[np.searchsorted(allv, gv)] = gc
    wn[np.searchsorted(allv, wv)] = wc
    return np.repeat(allv, np.maximum(wn - gn, 0)), np.repeat(allv, np.maximum(gn - wn, 0))


def knn_from_records(rec, nq: int, k: int):
    """(rows [nq, k], dists [nq, k], counts [nq]) of the first k records per needle of a sorted list; places past the
    count are zero"""
    u = unpack(rec)
    counts = np.bincount(u[:, 0], minlength=nq)
    starts = np.r_[0, np.cumsum(counts)]
    rows = np.zeros((nq, k), np.int64)
    dists = np.zeros((nq, k), np.int64)
    pos = np.arange(len(u)) - starts[u[:, 0]]
    keep = pos < k
    rows[u[keep, 0], pos[keep]] = u[keep, 2]
    dists[u[keep, 0], pos[keep]] = u[keep, 1]
    return rows, dists, counts


# ---- fixtures -----------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Fixture:
    name: str
    rows: np.ndarray  # [n, 32] uint8
    needles: np.ndarray  # [nq, 32] uint8
    thresh: int
    target: str  # what the builder proved through the model
    planted: np.ndarray  # [m, 3] (needle, row, distance) of the pairs the builder placed, matches and near misses
    batches: tuple = ()  # (q0, q1) needle ranges that are ALSO searched on their own (other kernels for the same registers)
    reached: dict = dataclasses.field(default_factory=dict)  # the model's counts, for reports

    def ranges(self):
        return ((0, len(self.needles)),) + tuple(self.batches)


def _planted(p):
    return np.asarray(p, np.int64).reshape(-1, 3)


def _check_planted(fx: Fixture):
    p = fx.planted
    assert (dist(fx.rows[p[:, 1]], fx.needles[p[:, 0]]) == p[:, 2]).all(), fx.name
    return fx


def _covers(values, full) -> bool:
    return set(np.unique(values).tolist()) >= set(full)


def diagonal(nq: int = 600, thresh: int = 25, seed: int = 1) -> Fixture:
    """needle j is a near copy of row (1031 j) % n: every wave, row tile, register, half, column and field of each
    row-stationary kernel holds a match, over >= 2 workgroups and >= 2 needle chunks"""
    rng = np.random.default_rng([seed, nq, thresh])
    n = 3100
    rows = rand_rows(rng, n)
    needles = np.zeros((nq, 32), np.uint8)
    planted = []
    for j in range(nq):
        row = (1031 * j + 7) % n
        needles[j] = flip_in(rng, rows[row], j % thresh, 0, 256)
        planted.append((j, row, j % thresh))
    planted = _planted(planted)
    r, q = planted[:, 1], planted[:, 0]
    p3 = place_mfma3(r, q, n, nq)
    assert _covers(p3["wave"], range(4)) and _covers(p3["tile"], range(12)) and _covers(p3["g"], range(16))
    assert _covers(p3["half"], (0, 1)) and _covers(p3["r"], range(32)) and _covers(p3["field"], range(3))
    assert len(np.unique(p3["wg"])) >= 2 and len(np.unique(p3["chunk"])) >= 2
    classes = set(zip(p3["wave"].tolist(), p3["tile"].tolist(), p3["g"].tolist(), p3["half"].tolist()))
    p1 = place_mfma(r, q, n, nq)  # (thresholds > 40: the same needles on k_hamm256_mfma<6,3,4>)
    assert _covers(p1["wave"], range(4)) and _covers(p1["tile"], range(6)) and _covers(p1["g"], range(16))
    assert len(np.unique(p1["wg"])) >= 2 and len(np.unique(p1["chunk"])) >= 2 and _covers(p1["second"], (0, 1))
    ps = place_scan(r, q, n, nq)
    assert _covers(ps["slot"], range(8)) and len(np.unique(ps["wg"])) >= 2 and len(np.unique(ps["chunk"])) >= 2
    assert _covers(ps["pos"], range(4))
    reached = dict(pairs=len(planted), mfma3_row_classes=len(classes), mfma3_chunks=int(p3["chunk"].max()) + 1)
    if nq <= 512:
        pm = place_small(r, q, n, nq)
        assert _covers(pm["wave"], range(4)) and _covers(pm["field"], range(3)) and _covers(pm["g"], range(16))
        assert _covers(pm["acc"], range(launch_small(n, nq)["na"])) and len(np.unique(pm["wg"])) >= 2
        reached["small_accumulators"] = int(pm["acc"].max()) + 1
    return _check_planted(Fixture(f"diagonal_q{nq}", rows, needles, thresh,
                                  "one match per wave / tile / register / half / column / field, 2+ workgroups and chunks",
                                  planted, reached=reached))


def threshold_edges(thresh: int, seed: int = 2) -> Fixture:
    """pairs at distance thresh - 1 and thresh with the differing bits all in the first 128, all in the last 128, spread
    over both, and split so that the first 128 bits alone pass while the total does not"""
    rng = np.random.default_rng([seed, thresh])
    n, nq = 2000, 100
    rows = rand_rows(rng, n)
    needles = rand_rows(rng, nq)
    planted, kinds = [], []
    j = 0
    for rep in range(4):
        for d in (thresh - 1, thresh):
            if d > 256:
                continue
            for kind in ("first", "last", "both", "split"):
                row = int(rng.integers(0, n))
                if kind == "first" and d <= 128:
                    nd = flip_in(rng, rows[row], d, 0, 128)
                elif kind == "last" and d <= 128:
                    nd = flip_in(rng, rows[row], d, 128, 256)
                elif kind == "both":
                    nd = flip_in(rng, rows[row], d, 0, 256)
                elif kind == "split" and d == thresh and min(thresh - 1, 128) + 128 >= thresh:
                    d1 = min(thresh - 1, 128)  # passes on the first 128 bits alone
                    nd = flip_in(rng, flip_in(rng, rows[row], d1, 0, 128), thresh - d1, 128, 256)
                    assert dist128(rows[row], nd) < thresh
                else:
                    continue
                needles[j] = nd
                planted.append((j, row, d))
                kinds.append(kind)
                j += 1
    assert j <= nq
    planted = _planted(planted)
    under, at = int((planted[:, 2] < thresh).sum()), int((planted[:, 2] >= thresh).sum())
    assert under >= 4 and (at >= 4 or thresh == 257)
    assert thresh > 256 or "split" in kinds
    return _check_planted(Fixture(f"threshold_edges_t{thresh}", rows, needles, thresh,
                                  f"{under} planted pairs at thresh - 1, {at} at thresh", planted,
                                  reached=dict(under=under, at=at, kinds=sorted(set(kinds)))))


_CARRY_KINDS = ("match", "miss_first", "miss_split", "none")


def carry_hidden(thresh: int = 25, seed: int = 3) -> Fixture:
    """field 2 carries at the end (its needle matches the row) while fields 0 / 1 of the same register hold matches, near
    misses at distance thresh (on the first 128 bits: field 127; split: flagged field, total thresh), or nothing.  Each
    row exists three times (exact duplicates in other tiles): per-needle counts of 3, ties by row."""
    rng = np.random.default_rng([seed, thresh])
    b = thresh - 1
    n, nq = 5003, 192
    rows = rand_rows(rng, n)
    needles = rand_rows(rng, nq)
    patterns = [(a, c) for a in _CARRY_KINDS for c in _CARRY_KINDS if (a, c) != ("none", "none")]
    planted, regs = [], []
    free = rng.permutation(n).tolist()
    for idx in range(64):
        p, c = idx // 32, idx % 32
        pat = patterns[idx % len(patterns)]
        copies = [free.pop() for _ in range(3)]
        rows[copies[1]] = rows[copies[2]] = rows[copies[0]]
        R = rows[copies[0]]
        top = flip_in(rng, R, int(rng.integers(0, b + 1)), 0, 256)
        needles[(3 * p + 2) * 32 + c] = top
        planted += [((3 * p + 2) * 32 + c, r, int(dist(R, top))) for r in copies]
        for f, kind in enumerate(pat):
            if kind == "none":
                continue
            if kind == "match":
                nd = flip_in(rng, R, int(rng.integers(0, b + 1)), 0, 256)
            elif kind == "miss_first":
                nd = flip_in(rng, R, thresh, 0, 128)
            else:
                d1 = thresh // 2
                nd = flip_in(rng, flip_in(rng, R, d1, 0, 128), thresh - d1, 128, 256)
            needles[(3 * p + f) * 32 + c] = nd
            planted += [((3 * p + f) * 32 + c, r, int(dist(R, nd))) for r in copies]
        regs.append((p, c, copies[0], pat))
    planted = _planted(planted)
    hidden = near = 0
    for p, c, row, pat in regs:
        st = accumulator_model(rows[row], register_needles(needles, p, np.int64(c)), thresh)
        assert st.end_ge and st.fields[2] >= 128
        for f, kind in enumerate(pat):
            if kind == "match":
                assert st.fields[f] >= 128
                hidden += 1
            elif kind == "miss_first":
                assert st.fields[f] == 127
                near += 1
            elif kind == "miss_split":
                assert st.fields[f] >= 128
                near += 1
            else:
                assert st.fields[f] < 127
    assert {pat for *_, pat in regs} == set(patterns)
    assert route(n, nq, thresh, "mfma") == K_SMALL8 and route(n, nq, thresh, "mfma_rows") == K_MFMA3
    return _check_planted(Fixture(f"carry_hidden_t{thresh}", rows, needles, thresh,
                                  f"end value >= 2^24 in {len(regs)} registers x 3 duplicate rows; {hidden} matches and {near} "
                                  f"near misses at distance thresh in the fields under the carry", planted,
                                  reached=dict(registers=3 * len(regs), hidden_matches=hidden, near_misses=near)))


def _excursion(kind: str, thresh: int, seed: int) -> Fixture:
    """the packed sum goes over 2^24 and comes back: the top field's needle (tile 3p + 2)
      "mfma":  distance <= b - 32 on bits 0..63, bits 64..127 all different  (over after the fifth MFMA, back after the sixth)
      "block": distance b - 16 on bits 0..95, bits 96..127 all different     (over after the K block of bits 64..95 of the
               sixth MFMA, back after its last block)
    while the same column's needle of field 0 (or field 1) is at first-128-bit distance b (field 128: one record at
    distance b), b + 1 (field 127: none) or b - 1 (field 129); every column of a tile, rows in both register halves"""
    rng = np.random.default_rng([seed, thresh, kind == "mfma"])
    b = thresh - 1
    assert (33 <= thresh <= 40) if kind == "mfma" else (17 <= thresh <= 40)
    n = 5003
    rows = rand_rows(rng, n)
    variants = [(sf, delta, half) for sf in (0, 1) for delta in (0, 1, -1) for half in (0, 1)]
    nq = len(variants) * 96
    needles = rand_rows(rng, nq)
    planted, regs = [], []
    for p, (sf, delta, half) in enumerate(variants):
        row = ((p * 13 + 1) % (n // 32)) * 32 + int(reg_row((p * 5 + 3) % 16, half))
        R = rows[row]
        for c in range(32):
            if kind == "mfma":
                top = flip_in(rng, R, int(rng.integers(0, b - 32 + 1)), 0, 64)
                top = flipped(top, range(64, 128))
            else:
                top = flip_in(rng, R, b - 16, 0, 96)
                top = flipped(top, range(96, 128))
            needles[(3 * p + 2) * 32 + c] = top
            sens = flip_in(rng, R, b + delta, 0, 128)
            needles[(3 * p + sf) * 32 + c] = sens
            planted.append(((3 * p + sf) * 32 + c, row, b + delta))
        regs.append((p, row, sf, delta, half))
    planted = _planted(planted)
    reached = dict(registers=0, field0_128=0, field1_128=0, field_127=0, field_129=0)
    for p, row, sf, delta, half in regs:
        cols = np.arange(32)
        st = accumulator_model(np.broadcast_to(rows[row], (32, 32)), register_needles(needles, p, cols), thresh)
        assert not st.end_ge.any() and (st.fields[:, 2] < 128).all()
        if kind == "mfma":
            assert st.mfma_ge.all() and (st.partials[:, 9] >= TWO24).all() and (st.partials[:, 7] < TWO24).all()
        else:
            assert not st.mfma_ge.any() and (st.partials[:, 10] >= TWO24).all() and (st.partials[:, 9] < TWO24).all()
            assert st.block_ge.all()
        assert (st.fields[:, sf] == 128 - delta).all() and (st.fields[:, 1 - sf] < 127).all()
        assert int(row_reg(row & 31)[1]) == half
        reached["registers"] += 32
        reached["field0_128" if sf == 0 else "field1_128"] += 32 * (delta == 0)
        reached["field_127"] += 32 * (delta == 1)
        reached["field_129"] += 32 * (delta == -1)
    assert {int(row_reg(r & 31)[1]) for _, r, *_ in regs} == {0, 1}
    # the same registers on k_hamm256_small: five whole triples per call of <= 512 needles
    batches = ((0, 480), (480, 960), (960, nq))
    assert [route(n, q1 - q0, thresh, "mfma") for q0, q1 in batches] == [K_SMALL16, K_SMALL16, K_SMALL8]
    assert route(n, nq, thresh, "mfma") == K_MFMA3
    where = "an MFMA-end partial" if kind == "mfma" else "a block-level partial (no MFMA-end one)"
    return _check_planted(Fixture(
        f"excursion_{kind}_t{thresh}", rows, needles, thresh,
        f"{where} >= 2^24 in {reached['registers']} registers, end value < 2^24; field 0 = 128 in {reached['field0_128']}, "
        f"field 1 = 128 in {reached['field1_128']}, a field of 127 in {reached['field_127']}, of 129 in {reached['field_129']}",
        planted, batches=batches, reached=reached))


def excursion_mfma(thresh: int = 33, seed: int = 4) -> Fixture:
    return _excursion("mfma", thresh, seed)


def excursion_block(thresh: int = 25, seed: int = 5) -> Fixture:
    return _excursion("block", thresh, seed)


def needle_shapes(nq: int, thresh: int = 25, seed: int = 6) -> Fixture:
    """nq needles against 5003 rows: a match for the first and the last needle of every needle tile"""
    rng = np.random.default_rng([seed, nq, thresh])
    n = 5003
    rows = rand_rows(rng, n)
    needles = rand_rows(rng, nq)
    planted = []
    targets = rng.permutation(n - 2).tolist()
    for t in range(_cdiv(nq, 32)):
        for j in sorted({32 * t, min(32 * t + 31, nq - 1)}):
            row = n - 1 if j == nq - 1 else targets.pop()  # (the last needle meets the last, ragged, row)
            d = (t + j) % thresh
            needles[j] = flip_in(rng, rows[row], d, 0, 256)
            planted.append((j, row, d))
    planted = _planted(planted)
    assert _covers(planted[:, 0], [32 * t for t in range(_cdiv(nq, 32))] + [nq - 1])
    L3, L1 = launch_mfma3(n, nq), launch_mfma(n, nq)
    reached = dict(tiles=L1["n_tiles"], mfma_chunks=L1["chunks"], mfma_last_chunk_tiles=L1["last_chunk_tiles"],
                   mfma3_chunks=L3["chunks"], mfma3_pad_tiles=L3["pad_tiles"], scan_last_block=nq % 4,
                   kernels={p: KERNEL_NAMES[route(n, nq, thresh, p)] for p in PATHS})
    return _check_planted(Fixture(f"needle_shapes_q{nq}_t{thresh}", rows, needles, thresh,
                                  f"{len(planted)} matches on the first and last needle of {L1['n_tiles']} tiles", planted,
                                  reached=reached))


def ragged_rows(n: int, thresh: int = 25, seed: int = 7) -> Fixture:
    """n rows: matches on row 0, on the first row of the last tile and on the last row"""
    rng = np.random.default_rng([seed, n, thresh])
    nq = 100
    rows = rand_rows(rng, n)
    needles = rand_rows(rng, nq)
    planted = []
    for i, row in enumerate(sorted({0, (n - 1) // 32 * 32, n - 1})):
        for rep in range(3):
            j = 33 * rep + i  # a needle in each of three tiles
            d = (5 * rep + i) % thresh
            needles[j] = flip_in(rng, rows[row], d, 0, 256)
            planted.append((j, row, d))
    needles[99] = flip_in(rng, rows[n - 1], 1, 128, 256)
    planted.append((99, n - 1, 1))
    planted = _planted(planted)
    assert _covers(planted[:, 1], (0, (n - 1) // 32 * 32, n - 1))
    return _check_planted(Fixture(f"ragged_rows_n{n}", rows, needles, thresh,
                                  f"matches on rows 0, {(n - 1) // 32 * 32} and {n - 1} of {n}", planted,
                                  reached=dict(rows_in_last_tile=(n - 1) % 32 + 1)))


def real_zeros(thresh: int = 25, seed: int = 8) -> Fixture:
    """all-zero rows in the first tile and in the ragged last tile, an all-zero needle first and last, needles within
    thresh - 1 of zero and at thresh: real matches that look like the padding beside them (n and nq both ragged)"""
    rng = np.random.default_rng([seed, thresh])
    n, nq = 1229, 70
    rows = rand_rows(rng, n)
    needles = rand_rows(rng, nq)
    zero_rows = [3, 17, 1220, n - 1]
    rows[zero_rows] = 0
    z = np.zeros(32, np.uint8)
    close = {0: z, nq - 1: z, 40: flip_in(rng, z, thresh - 1, 0, 128), 41: flip_in(rng, z, thresh, 0, 128),
             68: flip_in(rng, z, thresh - 1, 128, 256), 33: flip_in(rng, z, thresh - 1, 0, 256),
             34: flip_in(rng, flip_in(rng, z, thresh // 2, 0, 128), thresh - thresh // 2, 128, 256)}
    planted = []
    for j, nd in close.items():
        needles[j] = nd
        planted += [(j, r, int(dist(z, nd))) for r in zero_rows]
    planted = _planted(planted)
    assert n % 32 and nq % 32 and nq % 4 and (n - 1) // 32 == 1220 // 32 and 17 // 32 == 0
    matches = int((planted[:, 2] < thresh).sum())
    assert matches == 5 * len(zero_rows)
    return _check_planted(Fixture(f"real_zeros_t{thresh}", rows, needles, thresh,
                                  f"{len(zero_rows)} zero rows x (2 zero needles + 3 within thresh - 1): {matches} records, 2 needles "
                                  f"at thresh; {32 - n % 32} padding rows and {32 - nq % 32} padding needles are zero too", planted,
                                  reached=dict(records_on_zero_rows=matches)))


def dense(thresh: int = 40, seed: int = 9) -> Fixture:
    """3072 rows x 1536 needles of one cluster (each the centre with < thresh / 2 flips): every pair matches -- all lanes,
    registers and fields, the carry everywhere, 4.7 M records (the record buffer starts at 2^22)"""
    rng = np.random.default_rng([seed, thresh])
    n, nq = 3072, 1536
    centre = to_bits(rand_rows(rng, 1))[0]
    kmax = (thresh - 1) // 2

    def cluster(m):
        bits = np.broadcast_to(centre, (m, 256)).copy()
        for i in range(m):
            bits[i, rng.choice(256, int(rng.integers(0, kmax + 1)), replace=False)] ^= 1
        return from_bits(bits)

    rows, needles = cluster(n), cluster(nq)
    planted = _planted([(0, 0, int(dist(rows[0], needles[0]))), (nq - 1, n - 1, int(dist(rows[n - 1], needles[nq - 1])))])
    assert 2 * kmax < thresh and n * nq > (1 << 22)
    if thresh <= PRE128_MAX_THRESH:  # a sample of registers: every field flagged, the end value over 2^24
        st = accumulator_model(rows[:64, None, :], register_needles(needles, 5, np.arange(32))[None], thresh)
        assert st.end_ge.all() and (st.fields >= 128).all()
    batches = ((0, 512),)  # 512 needles: k_hamm256_small<16> where the path has it
    return _check_planted(Fixture(f"dense_t{thresh}", rows, needles, thresh,
                                  f"all {n * nq} pairs match: {n * nq - (1 << 22)} records more than the buffer starts with",
                                  planted, batches=batches, reached=dict(records=n * nq)))


def small_streaming(n: int = 1_100_013, thresh: int = 40, seed: int = 10) -> Fixture:
    """n random rows x 512 needles; needle j is a near copy (distance j % 40) of a planted row, the planted rows cycling
    through classes: row tiles that k_hamm256_small<16> reaches through prefetch slot u = 0..3 of its first trip, tiles of
    its second trip (from row 1 048 576), the ragged last tile, and the rows on both sides of every 16 384-row border
    (the segments of a sharded handle).  Classes that n does not have fall away."""
    rng = np.random.default_rng([seed, n])
    nq = 512
    rows = rand_rows(rng, n)
    needles = np.zeros((nq, 32), np.uint8)
    L = launch_small(n, nq)
    tiles = np.arange(L["row_tiles"])
    k = tiles // L["stride"]
    pools = {}
    for u in range(4):
        pools[f"u{u}"] = tiles[(k & 3 == u) & (k >> 2 == 0)]
    pools["trip1"] = tiles[k >> 2 == 1]
    pools["last_tile"] = tiles[-1:]
    classes = {name: t for name, t in pools.items() if len(t)}
    borders = np.arange(SHARD_RUN, n, SHARD_RUN)
    names = list(classes) + (["border_lo", "border_hi"] if len(borders) else [])
    planted = []
    for j in range(nq):
        name = names[j % len(names)]
        if name == "border_lo":
            row = int(rng.choice(borders)) - 1
        elif name == "border_hi":
            row = int(rng.choice(borders))
        else:
            row = min(int(rng.choice(classes[name])) * 32 + int(rng.integers(0, 32)), n - 1)
        if name == "last_tile" and j % (2 * len(names)) < len(names):
            row = n - 1
        d = j % 40
        needles[j] = flip_in(rng, rows[row], d, 0, 256)
        planted.append((j, row, d))
    planted = _planted(planted)
    reached = dict(classes=names, grid=L["grid"])
    ps = place_small(planted[:, 1], planted[:, 0], n, nq)
    if n > (1 << 20):
        for sub in (97, 200, 512):  # every class within the first 97 / 200 needles too (NT = 4, 8)
            m = planted[:, 0] < sub
            assert _covers(ps["u"][m & (ps["trip"] == 0)], range(4)) and (ps["trip"][m] == 1).any()
            assert ps["last_tile"][m].any() and (planted[m, 1] == n - 1).any() and _covers(ps["wave"][m], range(4))
        assert L["grid"] == 2048 and n % 32
        reached.update(trip1_pairs=int((ps["trip"] == 1).sum()), u_pairs=[int(((ps["u"] == u) & (ps["trip"] == 0)).sum())
                                                                        for u in range(4)])
    return _check_planted(Fixture(f"small_streaming_n{n}", rows, needles, thresh,
                                  f"{nq} planted pairs over {', '.join(names)}", planted, reached=reached))


# name -> builder; PARAMS: the values a builder is run with (a parameter of one builder, not that many fixtures) -- a plain
# value is the builder's one argument, a tuple adds the threshold: the needle and row shapes run at 25 (the prefilter
# kernels: k_hamm256_small, k_hamm256_mfma3, k_hamm256_mfma<6,3,2> below three tiles) and at 41, where every count goes
# to k_hamm256_mfma<6,3,4> with its needle chunks of four tiles and both tails of its two-tile loop
BUILDERS = {"diagonal": diagonal, "threshold_edges": threshold_edges, "carry_hidden": carry_hidden,
            "excursion_mfma": excursion_mfma, "excursion_block": excursion_block, "needle_shapes": needle_shapes,
            "ragged_rows": ragged_rows, "real_zeros": real_zeros, "dense": dense, "small_streaming": small_streaming}
NEEDLE_COUNTS = (1, 31, 32, 33, 64, 65, 95, 96, 97, 128, 129, 257, 258, 259, 512, 513, 1100)
ROW_COUNTS = (1, 31, 33, 383, 385, 1535, 1537, 2049)
PARAMS = {"diagonal": (512, 600, (600, 41)),
          "threshold_edges": (1, 2, 17, 25, 32, 33, 39, 40, 41, 42, 128, 129, 256, 257),
          "carry_hidden": (25, 40),
          "excursion_mfma": (33, 40),
          "excursion_block": (17, 25, 33, 40),
          "needle_shapes": NEEDLE_COUNTS + tuple((q, 41) for q in NEEDLE_COUNTS),
          "ragged_rows": ROW_COUNTS + tuple((n, 41) for n in ROW_COUNTS),
          "real_zeros": (25, 41),
          "dense": (40, 41),
          "small_streaming": (1_100_013,)}
CASES = [(name, p) for name, ps in PARAMS.items() for p in ps]
SMALL_CASES = [(name, p) for name, p in CASES if name != "small_streaming"]


@functools.lru_cache(maxsize=4)
def build(name: str, param) -> Fixture:
    return BUILDERS[name](*param) if isinstance(param, tuple) else BUILDERS[name](param)


# ---- the soak's case generator (tools/fuzz_scan256.py draws its cases here) ------------------------------------------------
def soak_case(rng) -> dict:
    """one random case: an index of n_img media of `per` random rows each, and nq queries that are rows with a random number
    of flipped bits around the threshold (hits just under, at and just over it), rows of zeros, unrelated descriptors, or
    flips confined to one half.  Draws from rng in a fixed order: the same seed gives the same cases."""
    n_img = int(rng.integers(8, 400))
    per = int(rng.integers(20, 700))
    rows = rng.integers(0, 256, (n_img * per, 32), dtype=np.uint8)
    n = len(rows)
    max_dist = int(rng.choice([0, 1, 5, 24, 25, 29, 39, 40, 41, 60, 90]))
    nq = int(rng.choice([1, 31, 32, 33, 95, 96, 97, 500, 512, 513, 1200, int(rng.integers(1, 2000))]))
    q = rows[rng.integers(0, n, nq)].copy()
    bits = np.unpackbits(q, axis=1)
    for j in range(nq):
        kind = rng.integers(0, 10)
        if kind < 7:  # flips around the threshold, anywhere in the 256 bits
            k = int(np.clip(max_dist + rng.integers(-3, 4), 0, 256))
            pos = rng.choice(256, k, replace=False)
            bits[j, pos] ^= 1
        elif kind == 7:
            bits[j] = rng.integers(0, 2, 256)
        elif kind == 8:
            bits[j] = 0
        else:  # all flips in the first 128 bits / in the last 128 bits
            k = int(np.clip(max_dist + rng.integers(-2, 3), 0, 128))
            pos = rng.choice(128, k, replace=False) + (128 if rng.integers(0, 2) else 0)
            bits[j, pos] ^= 1
    q = np.packbits(bits, axis=1)
    return dict(n_img=n_img, per=per, rows=rows, n=n, max_dist=max_dist, nq=nq, queries=q, bits=bits)
