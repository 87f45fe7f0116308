"""Where a pair lands in the 64-bit matrix-core scan kernels (cbird_amd/csrc/hamm64_mfma.hip), a model of the prefilter's
bookkeeping, a plain reference of the scan, and seeded fixtures that put matches at chosen places of that layout.

Plain numpy, no GPU and nothing from cbird_amd: the model restates the kernels' layout and their pending-list rules (how
many descriptors, records and queue entries a launch needs where); it never decides what the right answer is -- that is
reference_records(), every pair compared on all 64 bits.

Layout (names of hamm64_mfma.hip):
  * wave W = 4 b + w of workgroup b owns slots [256 W, 256 W + 256): kHT = 8 tiles of 32 rows (`tile0` of each kernel);
    group k of a step is tiles 2k, 2k+1 (kG = 2); slots past n are hash 0, and a wave with no slot < n exits
    (prefilter_body, load_hay_words);
  * MFMA C/D layout: lane L holds needle column c = L & 31, half = L >> 5, and register g (0..15) of a tile is slot row
    (g & 3) + 8 (g >> 2) + 4 half of the tile (cd_row); register r of a group = 16 t + g for its tile t;
  * PRE (k_hamm64_mfma<true>, description Pre32): a step is two needle pairs, 128 needles from 64 p; field f of a
    register is needle 64 p + 32 f + c (`work` in prefilter_body), and a step whose second pair does not exist takes the
    first again (Pre32::last_op, the clamp of needle_loop); needles past nq are hash 0 (k_expand_needles).  A register
    is flagged when any field has popc(fold(slot) ^ fold(needle)) < thresh, fold(x) = lo32 ^ hi32 (Pre32::hay,
    NeedleScratch::fold); a flagged top field makes all four fields candidates (`drain` in prefilter_body);
  * FULL3 (k_hamm64_mfma3): a triple is 96 needles, field f = needle 96 p + 32 f + c, flagged per field on the full
    64 bits; the per-tile queue takes one field at a time, <= 16 registers x 64 lanes (handle_tile3, queue_drain);
  * FULL2 (k_hamm64_mfma<false>, threshold 65): pair p = needles 64 p + 32 f + c, two entries per register, <= 2048 per
    tile (handle_tile2, kQueue).
Prefilter bookkeeping (as the kernel stood at the commit that added this module; today's rules are `detect` and `drain`
in prefilter_body, which tests/test_scan_prefilter_events.py and test_scan_prefilter_items.py follow):
a group whose flags sit in ONE lane lists that lane's flagged registers (<= 32 descriptors) and does not drain;
several hit lanes are parked kParkLanes = 16 at a time, each listing
its flagged registers; a drain keeps npend & 63 descriptors; the pending list holds kOutOff / 2 = 640.  Up to the commit
that added this module a multi-lane group drained only AFTER each chunk (at >= 64 pending), so a chunk could land on
63 + 3 x 32 pending descriptors: 671.  Draining only BEFORE a chunk that might not fit is not enough either: a chunk
left at up to 639 and followed by one-lane groups reaches 671 too.  The kernel now drains before such a chunk AND once
the multi-lane group is done, so a chunk lands on <= 128 and one-lane groups start from <= 63.  prefilter_model() takes
each of the three rules.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

WAVE_ROWS = 256  # kHT * 32 slots per wave
WAVES_PER_WG = 4  # kWaves
TILES = 8  # kHT
PARK_LANES = 16  # kParkLanes
PEND_CAP = 640  # kOutOff / 2 = (kQueue - kParkLanes * 32 - 2 * kOutCap) / 2
FULL3_QUEUE = 16 * 64  # s_queue_ of k_hamm64_mfma3, words per wave
FULL2_QUEUE = 2048  # kQueue of k_hamm64_mfma<false>

M32 = np.uint64(0xFFFFFFFF)


def fold(x) -> np.ndarray:
    """the prefilter word lo32 ^ hi32"""
    x = np.asarray(x, np.uint64)
    return ((x & M32) ^ (x >> np.uint64(32))).astype(np.uint32)


def reg_row(g: int, half: int) -> int:
    """slot row (in its tile) of accumulator register g of a lane in `half`"""
    return (g & 3) + 8 * (g >> 2) + 4 * half


def row_reg(rit):
    """inverse of reg_row: (g, half) of row rit of a tile"""
    rit = np.asarray(rit)
    return (rit & 3) + 4 * (rit >> 3), (rit >> 2) & 1


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def prefilter_pairs_per_chunk(n: int, nq: int) -> int:
    """needle pairs per blockIdx.y chunk of one prefilter launch (launch_hamm64_scan_mfma, one launch, no siblings)"""
    n_pairs, wgs = _cdiv(nq, 64), _cdiv(n, WAVE_ROWS * WAVES_PER_WG)
    ppc = 512
    while ppc > 16 and wgs * _cdiv(n_pairs, ppc) < 8192:
        ppc >>= 1
    if _cdiv(n_pairs, ppc) > 65535:
        ppc = ((n_pairs + 65534) // 65535 + 1) & ~1
    return ppc


def pairs_below(a, b, thresh: int, block: int = 1024):
    """(i, j) of every popc(a[i] ^ b[j]) < thresh, ordered by j then i"""
    a, b = np.asarray(a), np.asarray(b)
    ii, jj = [], []
    for j0 in range(0, len(b), block):
        d = np.bitwise_count(b[j0:j0 + block, None] ^ a[None, :])
        j, i = np.nonzero(d < thresh)
        ii.append(i)
        jj.append(j + j0)
    if not ii:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(ii).astype(np.int64), np.concatenate(jj).astype(np.int64)


# ---- reference ----------------------------------------------------------------------------------------------------------
def reference_records(hashes, ids, needles, thresh: int, masks=None) -> np.ndarray:
    """every pair with hamm64 < thresh, id != 0, needle != 0 (and ((needle ^ hash) & mask) == 0 where masks are given) as
    sorted cbh_records needle << 39 | dist << 32 | id -- i.e. the multiset of (needle, dist, id) in lexicographic order"""
    h = np.asarray(hashes, np.uint64)
    ids = np.asarray(ids, np.uint32)
    q = np.asarray(needles, np.uint64)
    out = []
    block = max(1, (1 << 22) // max(1, len(h)))
    for j0 in range(0, len(q), block):
        qb = q[j0:j0 + block]
        x = qb[:, None] ^ h[None, :]
        d = np.bitwise_count(x)
        ok = (d < thresh) & (ids != 0)[None, :] & (qb != 0)[:, None]
        if masks is not None:
            ok &= (x & np.asarray(masks, np.uint64)[j0:j0 + block, None]) == 0
        j, i = np.nonzero(ok)
        out.append(((j + j0).astype(np.uint64) << np.uint64(39)) | (d[j, i].astype(np.uint64) << np.uint64(32))
                   | ids[i].astype(np.uint64))
    r = np.concatenate(out) if out else np.zeros(0, np.uint64)
    return np.sort(r)


def unpack(rec) -> np.ndarray:
    """cbh_records -> rows (needle, dist, id)"""
    r = np.asarray(rec, np.uint64)
    return np.stack([(r >> np.uint64(39)).astype(np.int64), ((r >> np.uint64(32)) & np.uint64(0x7F)).astype(np.int64),
                     (r & M32).astype(np.int64)], axis=1)


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


# ---- the prefilter's bookkeeping ----------------------------------------------------------------------------------------
@dataclasses.dataclass
class Event:
    """one group of one step of one wave instance (wave, needle chunk) whose flags are not all clear"""
    wave: int
    chunk: int
    step: int
    group: int
    lanes: dict  # hit lane -> flagged registers
    fields: int  # fields the drain re-checks (all four for a register whose top field is flagged)
    before: int  # pending descriptors when the group starts
    peak: int  # the most the group has pending at once
    after: int  # pending when the group is done (before the end-of-step drain)


@dataclasses.dataclass
class PrefilterModel:
    peak: int
    events: list
    pad_slot: int  # fold candidates with a padding slot (row >= n)
    pad_needle: int  # ... with a padding needle (index >= nq, or the repeated pair of a lone last pair)
    ppc: int

    def instances(self):
        """(wave, chunk) -> events of that wave instance, in order"""
        d = {}
        for e in self.events:
            d.setdefault((e.wave, e.chunk), []).append(e)
        return d


RULES = ("parent", "before_only", "kernel")


def group_pending(npend: int, regs_per_lane, rule: str):
    """(peak, pending after) of one group whose hit lanes (ascending) hold regs_per_lane flagged registers each, entered
    with npend pending, under a multi-lane drain rule (prefilter_model)"""
    if len(regs_per_lane) == 1:  # one lane: listed, never drained here
        return npend + regs_per_lane[0], npend + regs_per_lane[0]
    peak = npend
    for c0 in range(0, len(regs_per_lane), PARK_LANES):
        if rule != "parent" and npend + PARK_LANES * 32 > PEND_CAP:
            npend &= 63
        npend += sum(regs_per_lane[c0:c0 + PARK_LANES])
        peak = max(peak, npend)
        if rule == "parent" and npend >= 64:
            npend &= 63
    if rule == "kernel" and npend >= 64:
        npend &= 63
    return peak, npend


def prefilter_model(hashes, needles, thresh: int, rule: str = "parent") -> PrefilterModel:
    """k_hamm64_mfma<true>'s per-group hit lanes, flagged registers and pending descriptors for one launch, under the
    multi-lane drain rule `rule`: "parent" -- after each chunk once >= 64 are pending (before the fix: what a chunk
    demands on top of what the step has pending); "before_only" -- before a chunk that might not fit, never after;
    "kernel" -- the kernel's rule now: before a chunk that might not fit, and after the group once >= 64 are pending."""
    assert rule in RULES
    assert 1 <= thresh <= 32
    n, nq = len(hashes), len(needles)
    n_pairs = _cdiv(nq, 64)
    ppc = prefilter_pairs_per_chunk(n, nq)
    sf = np.zeros(_cdiv(n, WAVE_ROWS) * WAVE_ROWS, np.uint32)
    sf[:n] = fold(hashes)
    nf = np.zeros(n_pairs * 64, np.uint32)
    nf[:nq] = fold(needles)
    i, j = pairs_below(sf, nf, thresh)
    pad_slot, pad_needle = int((i >= n).sum()), int((j >= nq).sum())
    P = j // 64
    chunk = P // ppc
    rel = P - chunk * ppc
    field = (rel & 1) * 2 + (j % 64) // 32
    # a lone last pair is its own partner: its needles are fields 2 and 3 of the step as well (and fall out at qi >= nq)
    lone = (n_pairs % 2 == 1) & (P == n_pairs - 1)
    pad_needle += int(lone.sum())
    i = np.concatenate([i, i[lone]])
    j = np.concatenate([j, j[lone]])
    chunk = np.concatenate([chunk, chunk[lone]])
    rel = np.concatenate([rel, rel[lone]])
    field = np.concatenate([field, field[lone] + 2])
    W, rw = i // WAVE_ROWS, i % WAVE_ROWS
    tile, rit = rw // 32, rw % 32
    g, half = row_reg(rit)
    lane = (j % 32) + 32 * half
    reg = 16 * (tile % 2) + g
    key = np.stack([W, chunk, rel // 2, tile // 2, lane, reg], axis=1)
    if len(key):
        uk, inv = np.unique(key, axis=0, return_inverse=True)
        bits = np.zeros(len(uk), np.int64)
        np.bitwise_or.at(bits, inv.reshape(-1), (1 << field).astype(np.int64))
    else:
        uk, bits = np.zeros((0, 6), np.int64), np.zeros(0, np.int64)
    nfields = np.where(bits & 8, 4, np.bitwise_count(bits & 7))
    events, peak = [], 0
    gk = uk[:, :4]
    starts = np.nonzero(np.r_[True, (gk[1:] != gk[:-1]).any(axis=1)])[0] if len(uk) else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], len(uk)]
    npend, inst, cur_step = 0, None, None
    for s, e in zip(starts.tolist(), ends.tolist()):
        Wv, cv, st, gr = (int(x) for x in gk[s])
        if (Wv, cv) != inst:
            inst, cur_step, npend = (Wv, cv), st, 0  # drain(true) at the end of a chunk
        elif st != cur_step:
            cur_step = st
            if npend >= 64:  # the end-of-step drain of every step in between
                npend &= 63
        lv, lc = np.unique(uk[s:e, 4], return_counts=True)
        lanes = dict(zip(lv.tolist(), lc.tolist()))
        before = npend
        gpeak, npend = group_pending(npend, lc.tolist(), rule)
        peak = max(peak, gpeak)
        events.append(Event(Wv, cv, st, gr, lanes, int(nfields[s:e].sum()), before, gpeak, npend))
    return PrefilterModel(peak, events, pad_slot, pad_needle, ppc)


def full3_queue(hashes, needles, thresh: int) -> dict:
    """k_hamm64_mfma3: (wave, tile, triple, field) -> queue entries of that pass (flagged registers x lanes)"""
    n, nq = len(hashes), len(needles)
    sh = np.zeros(_cdiv(n, WAVE_ROWS) * WAVE_ROWS, np.uint64)
    sh[:n] = hashes
    qh = np.zeros(_cdiv(nq, 96) * 96, np.uint64)
    qh[:nq] = needles
    i, j = pairs_below(sh, qh, thresh)
    k = np.stack([i // 32, j // 96, (j % 96) // 32], axis=1)
    if not len(k):
        return {}
    uk, cnt = np.unique(k, axis=0, return_counts=True)
    return {(int(a) // TILES, int(a) % TILES, int(b), int(c)): int(x) for (a, b, c), x in zip(uk, cnt)}


def full2_queue(hashes, needles, thresh: int) -> dict:
    """k_hamm64_mfma<false>: (wave, tile, pair) -> queue entries (two per register, one per needle tile)"""
    n, nq = len(hashes), len(needles)
    sh = np.zeros(_cdiv(n, WAVE_ROWS) * WAVE_ROWS, np.uint64)
    sh[:n] = hashes
    qh = np.zeros(_cdiv(nq, 64) * 64, np.uint64)
    qh[:nq] = needles
    i, j = pairs_below(sh, qh, thresh)
    k = np.stack([i // 32, j // 64], axis=1)
    if not len(k):
        return {}
    uk, cnt = np.unique(k, axis=0, return_counts=True)
    return {(int(a) // TILES, int(a) % TILES, int(b)): int(x) for (a, b), x in zip(uk, cnt)}


# ---- fixtures -----------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Fixture:
    name: str
    hashes: np.ndarray  # u64, load order
    ids: np.ndarray  # u32 (0 = removed slot)
    needles: np.ndarray  # u64 (0 = null needle)
    thresh: int
    masks: np.ndarray | None = None  # per-needle bits of (needle ^ hash) that must be zero
    prefilter: bool = False  # built for the prefilter kernel: the GPU test checks that it took the launch
    target: dict = dataclasses.field(default_factory=dict)  # what the builder asserted through the model


def _rand64(rng, k: int) -> np.ndarray:
    x = rng.integers(0, 1 << 63, k, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, k, dtype=np.uint64)
    x[x == 0] = 1 << 33
    return x


def _near(rng, base, k: int, flips_max: int) -> np.ndarray:
    """k copies of `base` with 0..flips_max distinct bits flipped"""
    out = np.full(k, base, np.uint64)
    for i in range(k):
        for b in rng.choice(64, int(rng.integers(0, flips_max + 1)), replace=False):
            out[i] ^= np.uint64(1) << np.uint64(int(b))
    return out


def _clean_fillers(rng, slots, needles, free_s, free_n, thresh: int, tries: int = 40) -> None:
    """re-draw filler slots / needles (free_*) until none of them is a fold candidate of anything, padding (hash 0)
    included; fixed entries keep their values (in place)"""
    for _ in range(tries):
        i, j = pairs_below(fold(slots), fold(needles), thresh)
        bad = free_s[i] | free_n[j]
        bs = np.unique(np.where(free_s[i[bad]], i[bad], -1))
        bn = np.unique(np.where(~free_s[i[bad]], j[bad], -1))
        bs = np.union1d(bs[bs >= 0], np.nonzero(free_s & (np.bitwise_count(fold(slots)) < thresh))[0])
        bn = np.union1d(bn[bn >= 0], np.nonzero(free_n & (np.bitwise_count(fold(needles)) < thresh))[0])
        if not len(bs) and not len(bn):
            return
        slots[bs] = _rand64(rng, len(bs))
        needles[bn] = _rand64(rng, len(bn))
    raise AssertionError("fillers did not come clean")


def _peak_wave_slots(X, Y, Z, nz: int, rand) -> np.ndarray:
    """one wave's 256 slots of the pending-peak pattern (rand: 256 filler hashes)"""
    s = rand.copy()
    r = np.arange(WAVE_ROWS)
    bit2 = ((r % 32) >> 2) & 1
    s[(r < 192) & (bit2 == 0)] = X  # tiles 0-5, rows a half-0 lane sees: X
    zrows = np.nonzero((r < 64) & (bit2 == 1))[0][:nz]  # tiles 0-1, rows of the half-1 lanes: nz of them Z
    s[zrows] = Z
    s[192:] = Y  # tiles 6-7: Y
    return s


def _peak_block_needles(X, Y, Z, nz: int, rand) -> np.ndarray:
    """a 256-needle block (two prefilter steps) of the pending-peak pattern"""
    q = rand.copy()
    q[5] = X  # step 0, field 0, lane 5: 32 registers in groups 0, 1, 2
    if nz:
        q[73] = Z  # step 0, field 2, column 9 -- lane 41 in group 0: group 0 has two hit lanes
    q[133] = X  # step 1, field 0, lane 5: three one-lane groups
    q[160:176] = Y  # step 1, field 1, columns 0..15 -- lanes 0..15 and 32..47 in group 3: two chunks of 16 hit lanes
    return q


@functools.lru_cache(maxsize=None)
def prefilter_pending_peak(remainder: int = 63, waves=(0,), blocks=(0,), n_waves: int | None = None,
                           nq: int | None = None, seed: int = 1) -> Fixture:
    """The prefilter's pending list at its worst: threshold 4, a wave instance whose step 0 ends with `remainder`
    descriptors kept (32 + the Z count), then step 1 lists 3 one-lane groups of 32 (remainder + 96) and a chunk of 16 hit
    lanes x 32 registers: a peak of 608 + remainder -- 640 = exactly the list's capacity for remainder 32, 671 for 63.
    The pattern sits in every wave of `waves` and every 256-needle block of `blocks` (block 4 = the first two steps of
    needle chunk 1: small launches cut needles in chunks of 16 pairs); everything else is a filler that is nobody's
    fold candidate, so no other wave instance has an event and the pattern's state does not depend on the chunking."""
    assert 32 <= remainder <= 63
    nz = remainder - 32
    thresh = 4
    rng = np.random.default_rng(seed)
    n_waves = n_waves or max(waves) + 1
    nq = nq or 256 * (max(blocks) + 1)
    assert all(256 * (b + 1) <= nq for b in blocks)
    X, Y, Z = _rand64(rng, 3)
    slots = _rand64(rng, n_waves * WAVE_ROWS)
    needles = _rand64(rng, nq)
    free_s, free_n = np.ones(len(slots), bool), np.ones(nq, bool)
    for w in waves:
        sl = slice(w * WAVE_ROWS, (w + 1) * WAVE_ROWS)
        pat = _peak_wave_slots(X, Y, Z, nz, np.zeros(WAVE_ROWS, np.uint64))
        slots[sl] = np.where(pat != 0, pat, slots[sl])
        free_s[sl] = pat == 0
    for b in blocks:
        sl = slice(b * 256, (b + 1) * 256)
        pat = _peak_block_needles(X, Y, Z, nz, np.zeros(256, np.uint64))
        needles[sl] = np.where(pat != 0, pat, needles[sl])
        free_n[sl] = pat == 0
    _clean_fillers(rng, slots, needles, free_s, free_n, thresh)
    ids = np.arange(1, len(slots) + 1, dtype=np.uint32)
    m = prefilter_model(slots, needles, thresh)
    ppc = m.ppc
    want = {(w, b * 256 // (64 * ppc)) for w in waves for b in blocks}
    inst = m.instances()
    assert set(inst) == want, ("events outside the pattern", sorted(set(inst) ^ want))
    assert all((b * 256) % (64 * ppc) == 0 for b in blocks), "a pattern block must start its needle chunk"
    for key, evs in inst.items():
        trace = [(e.step, e.group, len(e.lanes), e.before, e.peak, e.after) for e in evs]
        first = [(0, 0, 2 if nz else 1, 0, 32 + nz, 32 + nz), (0, 1, 1, 32 + nz, 64 + nz, 64 + nz),
                 (0, 2, 1, 64 + nz, 96 + nz, 96 + nz)]
        r = remainder
        second = [(1, 0, 1, r, r + 32, r + 32), (1, 1, 1, r + 32, r + 64, r + 64), (1, 2, 1, r + 64, r + 96, r + 96),
                  (1, 3, 32, r + 96, r + 96 + 512, (((r + 96 + 512) & 63) + 512) & 63)]
        assert trace == first + second, (key, trace)
    assert m.peak == 608 + remainder
    return Fixture(f"pending_peak_r{remainder}" + ("" if (waves, blocks) == ((0,), (0,)) else "_repl"), slots, ids,
                   needles, thresh, prefilter=True,
                   target={"peak": m.peak, "instances": len(inst), "list_capacity": PEND_CAP})


@functools.lru_cache(maxsize=None)
def dense_all_fields(seed: int = 2) -> Fixture:
    """One group in which all 64 lanes x 32 registers x 4 fields are true matches at distance 0: 8192 records out of one
    group (the wave's record buffer holds 128: out_flush in the middle of drain) -- and full per-field queues of the
    three-field kernel (16 registers x 64 lanes) for four fields of two triples in both tiles.  Threshold 5."""
    rng = np.random.default_rng(seed)
    thresh = 5
    n, nq = 2 * WAVE_ROWS + 40, 384
    slots, needles = _rand64(rng, n), _rand64(rng, nq)
    H = _rand64(rng, 1)[0]
    slots[256 + 64:256 + 128] = H  # wave 1, group 1
    needles[128:256] = H  # step 1 (needles 128..255): every field of every lane
    free_s, free_n = slots != H, needles != H
    _clean_fillers(rng, slots, needles, free_s, free_n, thresh)
    ids = np.arange(1, n + 1, dtype=np.uint32)
    m = prefilter_model(slots, needles, thresh)
    (ev,) = m.events
    assert (ev.wave, ev.step, ev.group) == (1, 1, 1) and len(ev.lanes) == 64 and set(ev.lanes.values()) == {32}
    assert ev.fields == 8192 and m.peak <= PEND_CAP
    q3 = full3_queue(slots, needles, thresh)
    assert max(q3.values()) == FULL3_QUEUE and sum(v == FULL3_QUEUE for v in q3.values()) >= 6
    return Fixture("dense_all_fields", slots, ids, needles, thresh, prefilter=True,
                   target={"fields": ev.fields, "full3_queue": max(q3.values())})


@functools.lru_cache(maxsize=None)
def dense_field3_only(seed: int = 3) -> Fixture:
    """A dense group in which only FIELD 3 (needles 96..127 of the step, the field that flags by carrying into the f32
    exponent) is near: every flagged register makes all four fields candidates and three of them must be dropped.  Half
    of field 3's needles are true neighbours (0..3 flipped bits), half only share the fold (x ^ (r | r << 32))."""
    rng = np.random.default_rng(seed)
    thresh = 4
    n, nq = WAVE_ROWS, 256
    slots, needles = _rand64(rng, n), _rand64(rng, nq)
    H = _rand64(rng, 1)[0]
    slots[128:192] = _near(rng, H, 64, 1)  # group 2
    f3 = np.arange(128 + 96, 128 + 128)  # step 1, field 3
    needles[f3[:16]] = _near(rng, H, 16, 2)
    r = rng.integers(1, 1 << 32, 16, dtype=np.uint64)
    needles[f3[16:]] = H ^ (r | (r << np.uint64(32)))  # the same fold, 64-bit distance 2 popc(r)
    free_s = np.ones(n, bool)
    free_s[128:192] = False
    free_n = np.ones(nq, bool)
    free_n[f3] = False
    _clean_fillers(rng, slots, needles, free_s, free_n, thresh)
    m = prefilter_model(slots, needles, thresh)
    assert len(m.events) == 1 and (m.events[0].step, m.events[0].group) == (1, 2)
    ev = m.events[0]
    flagged = sum(ev.lanes.values())
    assert len(ev.lanes) >= 32 and ev.fields == 4 * flagged  # only the top field: all four re-checked
    ref = reference_records(slots, np.ones(n, np.uint32), needles, thresh)
    assert 0 < len(ref) < ev.fields // 4  # some true, the rest dropped
    return Fixture("dense_field3_only", slots, np.arange(1, n + 1, dtype=np.uint32), needles, thresh, prefilter=True,
                   target={"registers": flagged, "fields": ev.fields})


@functools.lru_cache(maxsize=None)
def full3_field_queue_full(seed: int = 4) -> Fixture:
    """Threshold 12 (the three-field kernel as shipped): one field of one triple near a whole tile -- its queue pass holds
    exactly 16 registers x 64 lanes -- while the triple's other two fields hold scattered neighbours."""
    rng = np.random.default_rng(seed)
    thresh = 12
    n, nq = 3 * WAVE_ROWS, 96 * 5 + 17
    slots, needles = _rand64(rng, n), _rand64(rng, nq)
    H = _rand64(rng, 1)[0]
    slots[256 + 96:256 + 128] = _near(rng, H, 32, 4)  # wave 1, tile 3
    needles[96 * 2 + 32:96 * 2 + 64] = _near(rng, H, 32, 4)  # triple 2, field 1
    needles[96 * 2 + 3] = _near(rng, H, 1, 5)[0]
    needles[96 * 2 + 70] = _near(rng, H, 1, 6)[0]
    q3 = full3_queue(slots, needles, thresh)
    assert q3[(1, 3, 2, 1)] == FULL3_QUEUE and max(q3.values()) == FULL3_QUEUE
    assert (1, 3, 2, 0) in q3 and (1, 3, 2, 2) in q3
    return Fixture("full3_field_queue_full", slots, np.arange(1, n + 1, dtype=np.uint32), needles, thresh,
                   target={"full3_queue": FULL3_QUEUE})


@functools.lru_cache(maxsize=None)
def second_tile_only(seed: int = 5) -> Fixture:
    """Groups in which only the SECOND tile hits: one-lane events on each register at the edges of the prefilter's two
    reduction chains (registers 16 | 17, 19 | 20, 31; the one-lane path parks registers 0..19 or 16..31) in both lane
    halves, one per step; then a step where all 64 lanes see a whole second tile (multi-lane, first tile silent)."""
    rng = np.random.default_rng(seed)
    thresh = 4
    regs = [16, 17, 19, 20, 31]
    events = [(k, r, half) for k, (r, half) in enumerate((r, h) for r in regs for h in (0, 1))]
    n, nq = 3 * WAVE_ROWS, 128 * (len(events) + 1)
    slots, needles = _rand64(rng, n), _rand64(rng, nq)
    free_s, free_n = np.ones(n, bool), np.ones(nq, bool)
    hs = _rand64(rng, len(events) + 1)
    want = []
    for e, (k, r, half) in enumerate(events):
        group = k % 4
        g = r - 16
        s = 256 * (e % 2) + 32 * (2 * group + 1) + reg_row(g, half)
        f, c = e % 4, (7 * e) % 32
        slots[s], needles[128 * e + 32 * f + c] = hs[e], _near(rng, hs[e], 1, 3)[0]
        free_s[s], free_n[128 * e + 32 * f + c] = False, False
        want.append((e % 2, e, group, c + 32 * half, r))
    last = len(events)
    dt = slice(2 * WAVE_ROWS + 32 * 5, 2 * WAVE_ROWS + 32 * 6)  # wave 2, tile 5 = second tile of group 2
    slots[dt] = hs[last]
    needles[128 * last + 64:128 * last + 96] = hs[last]  # field 2 of the last step
    free_s[dt], free_n[128 * last + 64:128 * last + 96] = False, False
    _clean_fillers(rng, slots, needles, free_s, free_n, thresh)
    m = prefilter_model(slots, needles, thresh)
    dense = [e for e in m.events if len(e.lanes) > 1]
    got = sorted((e.wave, e.chunk, e.step, e.group, *e.lanes.items()) for e in m.events if len(e.lanes) == 1)
    spc = m.ppc // 2  # steps per needle chunk
    assert got == sorted((w, s // spc, s % spc, gr, (L, 1)) for w, s, gr, L, r in want), got
    assert len(dense) == 1
    dense = dense[0]
    assert (dense.wave, dense.chunk * spc + dense.step, dense.group, len(dense.lanes)) == (2, last, 2, 64)
    assert set(dense.lanes.values()) == {16}
    q3 = full3_queue(slots, needles, thresh)
    assert all(t % 2 == 1 for (_, t, _, _) in q3)  # the three-field kernel too: only odd tiles
    return Fixture("second_tile_only", slots, np.arange(1, n + 1, dtype=np.uint32), needles, thresh, prefilter=True,
                   target={"one_lane_events": len(events), "dense_lanes": 64})


@functools.lru_cache(maxsize=None)
def all_pairs_t65(seed: int = 6) -> Fixture:
    """Threshold 65: every pair is a match (FULL2: each per-tile queue is exactly 2048 entries, padding rows and needles
    included -- the guards drop those); removed slots and null needles among them."""
    rng = np.random.default_rng(seed)
    n, nq = 300, 130
    slots, needles = _rand64(rng, n), _rand64(rng, nq)
    slots[7] = 0  # a slot whose hash is 0
    ids = np.arange(1, n + 1, dtype=np.uint32)
    ids[[0, 31, 32, 299]] = 0
    needles[[0, 64, 129]] = 0
    q2 = full2_queue(slots, needles, 65)
    assert set(q2.values()) == {FULL2_QUEUE} and len(q2) == 2 * 8 * 3  # 2 waves x 8 tiles x 3 pairs, padding included
    return Fixture("all_pairs_t65", slots, ids, needles, 65, target={"full2_queue": FULL2_QUEUE})


@functools.lru_cache(maxsize=None)
def padding_guards(nq: int = 385, n: int = 2 * 1024 + 256 + 37, seed: int = 7) -> Fixture:
    """Slot and needle counts off every multiple (n not a multiple of 32, 256, 1024; nq = 1 mod 64, 96, 128, 192), dense
    tail rows equal to the last needle (which is alone in its pair, triple and step), and LOW-POPCOUNT slots and needles:
    the kernels pad both sides with hash 0, so a broken row < n / qi < nq guard shows up as a phantom match at
    distance popc(x)."""
    assert nq % 64 == 1 and nq % 96 == 1 and nq % 128 == 1 and nq % 192 == 1
    assert n % 32 and n % 256 and n % 1024
    rng = np.random.default_rng(seed)
    thresh = 4
    slots, needles = _rand64(rng, n), _rand64(rng, nq)
    low = np.array([1, 3, 1 << 40, (1 << 63) | 1, 7 << 20], np.uint64)  # popcount 1..3
    slots[rng.choice(n - 64, 40, replace=False)] = low[rng.integers(0, len(low), 40)]
    needles[rng.choice(nq - 1, 12, replace=False)] = low[rng.integers(0, len(low), 12)]
    H = _rand64(rng, 1)[0]
    tail = n % 32
    slots[n - tail:] = _near(rng, H, tail, 1)
    needles[nq - 1] = H
    ids = np.arange(1, n + 1, dtype=np.uint32)
    m = prefilter_model(slots, needles, thresh)
    assert m.pad_slot > 0 and m.pad_needle > 0
    # ... and on all 64 bits (the three-field kernel, the popcount kernel): low-popcount entries on both sides
    assert (np.bitwise_count(slots) < thresh).sum() >= 10 and (np.bitwise_count(needles) < thresh).sum() >= 5
    return Fixture(f"padding_n{n}_nq{nq}", slots, ids, needles, thresh, prefilter=True,
                   target={"pad_slot_candidates": m.pad_slot, "pad_needle_candidates": m.pad_needle})


@functools.lru_cache(maxsize=None)
def removed_null_masked(seed: int = 8) -> Fixture:
    """A dense cluster (many hit lanes in several groups) with removed slots (id 0), a slot whose hash is 0, null needles
    and per-needle masks: only slots equal to the needle on the masked bits qualify (find_batch(masks=...) -> mask_ok)."""
    rng = np.random.default_rng(seed)
    thresh = 5
    n, nq = 3 * WAVE_ROWS + 11, 512 + 3
    slots, needles = _rand64(rng, n), _rand64(rng, nq)
    H = _rand64(rng, 1)[0]
    slots[200:420] = _near(rng, H, 220, 3)
    needles[100:300] = _near(rng, H, 200, 3)
    needles[100:300:9] = 0  # null needles inside the dense steps
    slots[300] = 0
    needles[[7, 310]] = 1 << 2  # low-popcount needles: near the zero slot
    ids = np.arange(1, n + 1, dtype=np.uint32)
    ids[200:420:7] = 0  # removed slots inside the dense groups
    masks = np.zeros(nq, np.uint64)
    masks[1::2] = _rand64(rng, nq // 2) & np.uint64(0x00FF00FF00FF00FF)
    masks[::5] = np.uint64(0xFFFF)
    m = prefilter_model(slots, needles, thresh)
    assert max(len(e.lanes) for e in m.events) > PARK_LANES and m.peak <= PEND_CAP
    ref, refm = reference_records(slots, ids, needles, thresh), reference_records(slots, ids, needles, thresh, masks)
    assert 0 < len(refm) < len(ref)
    return Fixture("removed_null_masked", slots, ids, needles, thresh, masks=masks, prefilter=True,
                   target={"max_hit_lanes": max(len(e.lanes) for e in m.events)})


@functools.lru_cache(maxsize=None)
def join_wide_value(seed: int = 9) -> Fixture:
    """One chunk value shared by > 2048 needles and > 512 slots (the wide join splits it into jobs of 512 slots x 2048
    needles on both axes), made of EXACT duplicates -- every chunk of the join agrees on them, and only the first may report
    them -- plus near neighbours and fillers."""
    rng = np.random.default_rng(seed)
    H = _rand64(rng, 1)[0]
    slots = np.concatenate([np.full(600, H, np.uint64), _near(rng, H, 150, 7), _rand64(rng, 400)])
    needles = np.concatenate([np.full(2100, H, np.uint64), _near(rng, H, 200, 7), _rand64(rng, 300)])
    slots, needles = slots[rng.permutation(len(slots))], needles[rng.permutation(len(needles))]
    ids = np.arange(1, len(slots) + 1, dtype=np.uint32)
    ids[rng.choice(len(slots), 20, replace=False)] = 0
    needles[rng.choice(len(needles), 20, replace=False)] = 0
    assert (slots == H).sum() > 512 and (needles == H).sum() > 2048
    return Fixture("join_wide_value", slots, ids, needles, 6, target={"dup_slots": int((slots == H).sum()),
                                                                     "dup_needles": int((needles == H).sum())})


@functools.lru_cache(maxsize=None)
def prefilter_chunk_position(k: int, seed: int = 11) -> Fixture:
    """Every order of one multi-lane group among one-lane groups within a step: threshold 4, one wave, needles 0..255.
    Step 0 leaves 63 pending (needle 5 = A on 127 of the 128 rows the half-0 lanes see: four one-lane groups, 127).  In
    step 1 group k is a chunk of 16 hit lanes x 32 registers (needles 160..175 = C on the half-1 rows of group k) and the
    other three groups are one-lane with 32 registers (needle 192 = D on the half-1 rows of those groups).  The chunk
    meets 63 + 32 k pending: the parent's rule (drain after the chunk) overruns for k = 3 (671), draining only before a
    chunk overruns for k = 0..2 (the chunk stays, the one-lane groups behind it add up to 671); the kernel's rule keeps
    every order <= 640."""
    assert 0 <= k <= 3
    thresh = 4
    rng = np.random.default_rng(seed + k)
    A, C, D = _rand64(rng, 3)
    slots, needles = _rand64(rng, WAVE_ROWS), _rand64(rng, 256)
    r = np.arange(WAVE_ROWS)
    bit2, group = ((r % 32) >> 2) & 1, r // 64
    fixed_s = np.zeros(WAVE_ROWS, bool)
    a_rows = np.nonzero(bit2 == 0)[0][1:]  # 127 rows: step 0 ends with 127 pending, keeps 63
    slots[a_rows] = A
    slots[(bit2 == 1) & (group == k)] = C
    slots[(bit2 == 1) & (group != k)] = D
    fixed_s[a_rows] = True
    fixed_s[bit2 == 1] = True
    needles[5], needles[160:176], needles[192] = A, C, D
    fixed_n = np.zeros(256, bool)
    fixed_n[[5, 192]] = True
    fixed_n[160:176] = True
    _clean_fillers(rng, slots, needles, ~fixed_s, ~fixed_n, thresh)
    peaks = {rule: prefilter_model(slots, needles, thresh, rule).peak for rule in RULES}
    m = prefilter_model(slots, needles, thresh, "kernel")
    trace = [(e.step, e.group, len(e.lanes), e.before, e.peak) for e in m.events]
    want = [(0, 0, 1, 0, 31)] + [(0, g, 1, 31 + 32 * (g - 1), 63 + 32 * (g - 1)) for g in (1, 2, 3)]
    pend = 63
    for g in range(4):
        if g == k:
            start = pend if pend + 512 <= PEND_CAP else pend & 63
            want.append((1, g, 16, pend, start + 512))
            pend = (start + 512) & 63
        else:
            want.append((1, g, 1, pend, pend + 32))
            pend += 32
    assert trace == want, (k, trace)
    assert peaks["kernel"] <= PEND_CAP and peaks["parent"] == (671 if k == 3 else 63 + 32 * k + 512)
    assert peaks["before_only"] == (671 if k < 3 else 543)
    return Fixture(f"chunk_at_group{k}", slots, np.arange(1, WAVE_ROWS + 1, dtype=np.uint32), needles, thresh,
                   prefilter=True, target={"peaks": peaks})


def peak_replicated() -> Fixture:
    """the remainder-63 pattern in waves of both workgroups and in needle chunks 0 and 1 at once"""
    return prefilter_pending_peak(63, waves=(0, 3, 5, 6), blocks=(0, 4), n_waves=7, nq=1280 + 37)


BUILDERS = {
    "peak_r32": lambda: prefilter_pending_peak(32),
    "peak_r33": lambda: prefilter_pending_peak(33),
    "peak_r47": lambda: prefilter_pending_peak(47),
    "peak_r63": lambda: prefilter_pending_peak(63),
    "peak_repl": peak_replicated,
    "chunk_at_group0": lambda: prefilter_chunk_position(0),
    "chunk_at_group1": lambda: prefilter_chunk_position(1),
    "chunk_at_group2": lambda: prefilter_chunk_position(2),
    "chunk_at_group3": lambda: prefilter_chunk_position(3),
    "dense_all_fields": dense_all_fields,
    "dense_field3_only": dense_field3_only,
    "full3_field_queue_full": full3_field_queue_full,
    "second_tile_only": second_tile_only,
    "all_pairs_t65": all_pairs_t65,
    "padding_385": padding_guards,
    "padding_769": lambda: padding_guards(769, 1024 + 512 + 1, seed=17),
    "removed_null_masked": removed_null_masked,
    "join_wide_value": join_wide_value,
}
