"""The prefilter's drain by WORK ITEM (k_hamm64_mfma<true>, cbird_amd/csrc/hamm64_mfma.hip): a pending descriptor {flag
bits of a lane's two reduction chains, lane | group | step} becomes one item per candidate (chain, field) -- all four fields
of a chain whose top field carried -- and the wave works the items off 64 at a time, one per lane: its one needle against
the chain's 17 or 15 rows.  Whole batches only; fewer than 64 items wait for the next drain and for the end of the needle
chunk, as fewer than 64 descriptors do.

What that can get wrong: an item listed twice or not at all when lanes hold 8, 4 and 1 of them side by side, the list at
its capacity (63 kept + 64 x 8), the kept descriptors and the kept items around a non-final drain, a needle that matches
every row of its chain, a null needle and a padding needle among the items.  item_trace() restates the bookkeeping so that
each input is known to reach its case; the GPU tests compare the FULL record multiset with scan_layout.reference_records
and with the same call on the popcount kernel ("scan_mfma" 0).

n = 1024 (one workgroup), nq = 256 (two steps of one needle chunk), thresholds 6 and 7.  One input has nq = 250: with
256 needles every needle of both steps exists, and an item can name a needle >= nq only where the last step is short."""
import ctypes as C
import functools

import numpy as np
import pytest

import scan_layout as S

ITEM_CAP = 63 + 64 * 8  # kItemCap
THRESHOLDS = (6, 7)
N, NQ = 1024, 256


# ---- the rule, in numpy -------------------------------------------------------------------------------------------------
def descriptors(hashes, needles, thresh):
    """{(wave, chunk): {step: [(group, lane, cm)]}} in the order the kernel appends them (group, then lane): cm bit
    4 chain + f = field f is a candidate in the rows of chain `chain` (registers 0..16 | 17..31 of the group)"""
    n, nq = len(hashes), len(needles)
    n_pairs = S._cdiv(nq, 64)
    assert n_pairs % 2 == 0, "no lone last pair in these inputs"
    ppc = S.prefilter_pairs_per_chunk(n, nq)
    sf = np.zeros(S._cdiv(n, S.WAVE_ROWS) * S.WAVE_ROWS, np.uint32)
    sf[:n] = S.fold(hashes)
    nf = np.zeros(n_pairs * 64, np.uint32)
    nf[:nq] = S.fold(needles)
    i, j = S.pairs_below(sf, nf, thresh)
    P = j // 64
    chunk, rel = P // ppc, P % ppc
    field = (rel & 1) * 2 + (j % 64) // 32
    W, rw = i // S.WAVE_ROWS, i % S.WAVE_ROWS
    g, half = S.row_reg(rw % 32)
    lane = (j % 32) + 32 * half
    chain = (16 * ((rw // 32) % 2) + g > 16).astype(np.int64)
    flags = {}
    for k in zip(W.tolist(), chunk.tolist(), (rel // 2).tolist(), (rw // 64).tolist(), lane.tolist(), chain.tolist(),
                 field.tolist()):
        flags[k[:5]] = flags.get(k[:5], 0) | (1 << (4 * k[5] + k[6]))
    out = {}
    for (w, c, s, gr, ln), b in sorted(flags.items()):
        cm = sum((0xF if (b >> (4 * ch)) & 8 else (b >> (4 * ch)) & 7) << (4 * ch) for ch in (0, 1))
        out.setdefault((w, c), {}).setdefault(s, []).append((gr, ln, cm))
    return out


def item_trace(hashes, needles, thresh):
    """per wave instance: the items listed per pass of <= 64 descriptors, the batches worked, the most items the list
    held, the descriptors and items every non-final drain kept"""
    res = {}
    for inst, steps in descriptors(hashes, needles, thresh).items():
        t = {"listed": [], "batches": [], "peak": 0, "kept_desc": [], "kept_items": [], "items": 0}
        pend, nitem = [], 0

        def drain(final):
            nonlocal pend, nitem
            keep = 0 if final else len(pend) & 63
            k0 = keep
            while True:
                if nitem < 64 and k0 < len(pend):
                    c = sum(int(cm).bit_count() for cm in pend[k0:k0 + 64])
                    nitem += c
                    t["listed"].append(c)
                    t["items"] += c
                    t["peak"] = max(t["peak"], nitem)
                    k0 += 64
                elif nitem >= 64:
                    nitem -= 64
                    t["batches"].append(64)
                elif final and nitem:
                    t["batches"].append(nitem)
                    nitem = 0
                else:
                    break
            pend = pend[:keep]
            if not final:
                t["kept_desc"].append(keep)
                t["kept_items"].append(nitem)

        for s in sorted(steps):
            pend += [cm for _, _, cm in steps[s]]
            assert len(pend) <= 319
            if len(pend) >= 64:
                drain(False)
        drain(True)
        res[inst] = t
    return res


# ---- inputs: wave 0, rows of one group per step ------------------------------------------------------------------------
def _row(group, tile, reg, half):
    """wave row of register `reg` (0..15) of tile `tile` (0 | 1) of a group, for a lane in `half`"""
    return 64 * group + 32 * tile + S.reg_row(reg, half)


def _build(name, thresh, seed, plant, nq=NQ):
    rng = np.random.default_rng(seed)
    slots, needles = S._rand64(rng, N), S._rand64(rng, nq)
    fs, fn = np.zeros(N, bool), np.zeros(nq, bool)

    def slot(row, v):
        slots[row], fs[row] = v, True

    def needle(j, v):
        needles[j], fn[j] = v, True

    plant(rng, slot, needle)
    S._clean_fillers(rng, slots, needles, ~fs, ~fn, thresh)
    return S.Fixture(f"{name}_t{thresh}", slots, np.arange(1, N + 1, dtype=np.uint32), needles, thresh, prefilter=True)


ONE = np.uint64(1)


@functools.lru_cache(maxsize=None)
def mixed_loads(thresh):
    """one group, 64 hit lanes: 16 with the top field's carry in both chains (8 items), 16 with it in one (4), 32 with one
    field of one chain (1) -- 224 items of one pass: three batches of 64, and 32 that wait for the chunk's end.  Behind
    the carries sit true matches in a lower field."""
    def plant(rng, slot, needle):
        A, B, E, F = S._rand64(rng, 4)
        slot(_row(0, 0, 0, 0), A)          # half 0, chain 0
        slot(_row(0, 1, 1, 0), A ^ ONE)    # half 0, chain 1 (register 17)
        slot(_row(0, 0, 1, 0), E)          # half 0, chain 0
        slot(_row(0, 0, 0, 1), B)          # half 1, chain 0
        slot(_row(0, 0, 1, 1), F)          # half 1, chain 0
        for c in range(16):
            needle(96 + c, A)              # lane (c, 0): top field in both chains
            needle(32 + c, A ^ ONE)        # ... and a match behind the carry
            needle(c, F)                   # lane (c, 1): field 0, chain 0
        for c in range(16, 32):
            needle(32 + c, E)              # lane (c, 0): field 1, chain 0
            needle(96 + c, B)              # lane (c, 1): top field, chain 0
    return _build("mixed_loads", thresh, 41, plant)


@functools.lru_cache(maxsize=None)
def list_full(thresh):
    """step 0 lists 127 items (9 lanes x 8, 55 x 1) and keeps 63; step 1 is the maximum, 64 descriptors x 8 items: the
    list holds 63 + 512 = its capacity"""
    def plant(rng, slot, needle):
        P, Q, R, A = S._rand64(rng, 4)
        slot(_row(1, 0, 0, 0), P)
        slot(_row(1, 1, 1, 0), P ^ ONE)
        slot(_row(1, 0, 1, 0), Q)
        slot(_row(1, 0, 0, 1), R)
        for c in range(9):
            needle(96 + c, P)
        for c in range(9, 32):
            needle(c, Q)
        for c in range(32):
            needle(32 + c, R)
        for half in (0, 1):
            slot(_row(0, 0, 0, half), A)
            slot(_row(0, 1, 1, half), A)
        for c in range(32):
            needle(128 + 96 + c, A)
    return _build("list_full", thresh, 42, plant)


@functools.lru_cache(maxsize=None)
def kept_remainder(thresh):
    """step 0 ends with 127 descriptors: the non-final drain works the newest 64 and keeps 63, the final one takes them"""
    def plant(rng, slot, needle):
        P, R, S1, S2 = S._rand64(rng, 4)
        slot(_row(0, 0, 0, 0), P)
        slot(_row(0, 0, 0, 1), R)
        slot(_row(1, 0, 0, 0), S1)
        slot(_row(1, 1, 5, 1), S2)  # chain 1
        for c in range(32):
            needle(c, P)
            needle(32 + c, R)
            needle(64 + c, S1)
        for c in range(31):
            needle(96 + c, S2)
    return _build("kept_remainder", thresh, 43, plant)


@functools.lru_cache(maxsize=None)
def whole_chains(thresh):
    """needle X equals all 17 + 15 rows lane (7, half 0) sees in group 2, needle Y (top field) all rows of lane (9, half 1)"""
    def plant(rng, slot, needle):
        X, Y = S._rand64(rng, 2)
        for tile in (0, 1):
            for reg in range(16):
                slot(_row(2, tile, reg, 0), X)
                slot(_row(2, tile, reg, 1), Y)
        needle(128 + 32 + 7, X)
        needle(128 + 96 + 9, Y)
    return _build("whole_chains", thresh, 44, plant)


@functools.lru_cache(maxsize=None)
def null_and_padding_needles(thresh):
    """nq = 250.  Slot Z has fold 0 and is 32 bits from hash 0: a candidate of the null needles (fields 1 and 2 of step 0)
    and of the padding needles 250..255 (top field of step 1: four items each, three of them real needles); slot A's
    needle carries in the top field above a null needle"""
    def plant(rng, slot, needle):
        Z = np.uint64(0x00FF00FF00FF00FF)
        A = S._rand64(rng, 1)[0]
        slot(_row(3, 1, 2, 1), Z)
        slot(_row(1, 0, 3, 0), A)
        needle(32 + 5, 0)
        needle(64 + 20, 0)
        needle(128 + 96 + 3, A)
        needle(128 + 3, 0)
        needle(128 + 32 + 3, A ^ ONE)
    fx = _build("null_and_padding_needles", thresh, 45, plant, nq=250)
    assert np.bitwise_count(S.fold(np.array([0x00FF00FF00FF00FF], np.uint64)))[0] == 0
    return fx


FIXTURES = {"mixed_loads": mixed_loads, "list_full": list_full, "kept_remainder": kept_remainder,
            "whole_chains": whole_chains, "null_and_padding_needles": null_and_padding_needles}


# ---- CPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thresh", THRESHOLDS)
def test_inputs_reach_their_cases(thresh):
    tr = {k: item_trace(f(thresh).hashes, f(thresh).needles, thresh) for k, f in FIXTURES.items()}
    ref = {k: S.unpack(S.reference_records(f(thresh).hashes, f(thresh).ids, f(thresh).needles, thresh))
           for k, f in FIXTURES.items()}
    for k, v in tr.items():
        assert set(v) == {(0, 0)}, k  # wave 0, one needle chunk; the fillers are nobody's candidates
        assert v[(0, 0)]["peak"] <= ITEM_CAP
        assert sum(v[(0, 0)]["batches"]) == v[(0, 0)]["items"]

    t = tr["mixed_loads"][(0, 0)]
    d = descriptors(mixed_loads(thresh).hashes, mixed_loads(thresh).needles, thresh)[(0, 0)]
    assert sorted(int(cm).bit_count() for _, _, cm in d[0]) == [1] * 32 + [4] * 16 + [8] * 16
    assert t["listed"] == [224] and t["batches"] == [64, 64, 64, 32] and t["kept_items"] == [32]
    # 16 x (A on two rows + A ^ 1 on two rows) + 16 E + 16 B + 16 F
    assert len(ref["mixed_loads"]) == 16 * 4 + 48

    t = tr["list_full"][(0, 0)]
    assert t["listed"] == [127, 512] and t["peak"] == ITEM_CAP
    assert t["batches"] == [64] + [64] * 8 + [63] and t["kept_items"] == [63, 63]
    assert len(ref["list_full"]) == 9 * 2 + 23 + 32 + 32 * 4

    t = tr["kept_remainder"][(0, 0)]
    assert t["kept_desc"] == [63] and len(t["listed"]) == 2 and t["items"] == 64 + 32 + 31 * 4
    assert len(ref["kept_remainder"]) == 32 * 3 + 31

    assert len(ref["whole_chains"]) == 64
    assert (ref["whole_chains"][:, 0] == 128 + 32 + 7).sum() == 32 and (ref["whole_chains"][:, 1] == 0).all()

    fx = null_and_padding_needles(thresh)
    d = descriptors(fx.hashes, fx.needles, thresh)[(0, 0)]
    lanes0 = {ln: cm for g, ln, cm in d[0] if g == 3}
    assert lanes0 == {32 + 5: 0x20, 32 + 20: 0x40}  # the null needles: one item each, chain 1
    lanes1 = {ln: cm for g, ln, cm in d[1] if g == 3}
    assert lanes1 == {32 + 3: 0x10, **{32 + c: 0xF0 for c in range(26, 32)}}  # a null needle, the padding needles 250..255
    assert {ln: cm for g, ln, cm in d[1] if g == 1} == {3: 0x0F}
    assert [tuple(x) for x in ref["null_and_padding_needles"].tolist()] == [
        (128 + 32 + 3, 1, _row(1, 0, 3, 0) + 1), (128 + 96 + 3, 0, _row(1, 0, 3, 0) + 1)]


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def _scan(L, idx, needles, thresh, cap):
    import torch

    from cbird_amd import _lib

    dq = torch.from_numpy(needles.view(np.int64)).cuda()
    drec = torch.zeros(max(1, cap), dtype=torch.int64, device="cuda")
    dtot = torch.zeros(1, dtype=torch.int64, device="cuda")
    _lib.check(L.cbh_idx64_scan_dev(idx.handle, dq.data_ptr(), len(needles), thresh, drec.data_ptr(), cap,
                                    dtot.data_ptr(), None), "scan")
    tot = int(dtot.item())
    v = C.c_longlong(0)
    assert L.cbh_get_tuning(b"scan_pre_mask", C.byref(v)) == 0
    return tot, np.sort(drec[:min(tot, cap)].cpu().numpy().view(np.uint64)), bool((v.value >> thresh) & 1)


def _same(name, got, want):
    if not np.array_equal(got, want):
        missing, extra = S.multiset_diff(got, want)
        raise AssertionError(f"{name}: {len(got)} records, {len(want)} expected; {len(missing)} missing "
                             f"{S.unpack(missing[:4]).tolist()}, {len(extra)} extra {S.unpack(extra[:4]).tolist()}")


@pytest.mark.gpu
@pytest.mark.parametrize("thresh", THRESHOLDS)
@pytest.mark.parametrize("name", list(FIXTURES))
def test_items_equal_the_popcount_kernel(gpu, name, thresh):
    from cbird_amd import _lib

    fx = FIXTURES[name](thresh)
    want = S.reference_records(fx.hashes, fx.ids, fx.needles, thresh)
    idx = gpu.DctHashIndex()
    idx.load(fx.hashes, fx.ids)
    cap = len(want) + 4096
    L = _lib.lib()
    try:
        assert L.cbh_set_tuning(b"scan_mfma", 2) == _lib.CBH_OK and L.cbh_set_tuning(b"scan_mfma_pre_max", 32) == _lib.CBH_OK
        tot, got, pre = _scan(L, idx, fx.needles, thresh, cap)
        assert pre, "not the prefilter kernel"
        assert L.cbh_set_tuning(b"scan_mfma", 0) == _lib.CBH_OK
        tot0, got0, _ = _scan(L, idx, fx.needles, thresh, cap)  # (the mask speaks of matrix-core launches only)
    finally:
        L.cbh_set_tuning(b"scan_mfma", 1)
        L.cbh_set_tuning(b"scan_mfma_pre_max", -1)
    _same(f"{fx.name} vs popcount kernel", got, got0)
    _same(f"{fx.name} vs reference", got, want)
    assert tot == tot0 == len(want)
