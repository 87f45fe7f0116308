"""The arithmetic of the 48-bit prefilter (PRE48, cbird_amd/csrc/hamm64_mfma.hip) on paper: scan48_layout.chain() models
the three chained MFMAs of one accumulator register; the flag rule is checked against plain popcounts.

The rule.  Field f ends at 32 + t - h_f (h_f = 48-bit distance of needle f), so its bit 5 says h_f <= t.  A field of
h > 32 + t is negative: it borrows one from the field above (which then says h <= t - 1) and itself reads as flagged.
What the kernel needs is one-sided: every pair with hamm64 < t must be a candidate; candidates beyond that only cost a
re-check.  Both are asserted: the exact reading where no field wraps, the one-sided one where one does."""
import numpy as np
import pytest

import scan48_layout as M

THRESHOLDS = (1, 7, 8, 16)


def _rand64(rng, k):
    return [int(x) for x in rng.integers(0, 1 << 64, k, dtype=np.uint64)]


def _far(rng, row, t):
    """a needle whose 48-bit distance from `row` is well above t and at most 32 (no flag, no wrap)"""
    while True:
        x = _rand64(rng, 1)[0]
        if t + 2 <= M.popc48(row, x) <= 32:
            return x


def test_layout_tables_cover_every_field_once():
    """the twelve needle sub-blocks meet the haystack's windows element for element, and every element of field f weighs
    64^f / 2"""
    for m in range(3):
        for kb in range(2):
            for j in range(2):
                e, mag = M.HAY[kb][m + j]
                slot = 2 * (2 * m + kb) + j
                assert e == slot % 3
                nmag = M.FOUR if slot in M.NEEDLE_FOUR else M.HALF
                assert mag * nmag * M.SCALES[m][kb] == 64.0 ** (slot // 3) / 2
    # the top field arrives in the last MFMA only
    assert all(2 * (2 * m + kb) + j < 9 for m in range(2) for kb in range(2) for j in range(2))


def test_bound_popc48_le_hamm64():
    rng = np.random.default_rng(1)
    a, b = _rand64(rng, 4000), _rand64(rng, 4000)
    assert all(M.popc48(x, y) <= M.hamm64(x, y) for x, y in zip(a, b))
    # both bits of a folded pair: two bits of distance the word does not see
    for x in a[:200]:
        for i in range(16):
            y = x ^ (1 << i) ^ (1 << (i + 32))
            assert M.popc48(x, y) == 0 and M.hamm64(x, y) == 2
    # near pairs, where the bound is tight
    for x in a[:500]:
        y = x
        for i in rng.choice(64, 9, replace=False).tolist():
            y ^= 1 << i
        assert M.popc48(x, y) <= 9 == M.hamm64(x, y)


def test_c0_and_a_clean_chain_decode_to_the_distances():
    rng = np.random.default_rng(2)
    for t in THRESHOLDS:
        assert int(np.array([M.c0(t)]).view(np.uint32)[0]) & 0x7FFFFF == (8 + t) * M.FIELD_ONES
        for _ in range(50):
            row = _rand64(rng, 1)[0]
            nd = [_far(rng, row, t) for _ in range(4)]
            bits = M.chain(row, nd, t)
            assert bits >> 23 == 150  # the exponent of [2^23, 2^24)
            assert M.fields(bits) == [32 + t - M.popc48(row, x) for x in nd]
            assert M.candidates(bits) == 0


@pytest.mark.parametrize("t", THRESHOLDS)
@pytest.mark.parametrize("field", range(4))
@pytest.mark.parametrize("sub_block", range(3))
def test_boundary_distances_in_every_field_and_sub_block(t, field, sub_block):
    """h = t - 1, t, t + 1 with the differences confined to one sub-block, the other fields far: flagged iff h <= t"""
    rng = np.random.default_rng(100 * t + 10 * field + sub_block)
    for h in (t - 1, t, t + 1):
        if h > 16:
            continue  # a sub-block has 16 elements
        for _ in range(4):
            row = _rand64(rng, 1)[0]
            nd = [_far(rng, row, t) for _ in range(4)]
            nd[field] = M.flip(row, sub_block, h)
            assert M.popc48(row, nd[field]) == h == M.hamm64(row, nd[field])
            got = M.candidates(M.chain(row, nd, t))
            if h <= t:
                assert got & (1 << field), (t, field, sub_block, h)
                if field < 3:
                    assert got == 1 << field  # nothing else flagged
            else:
                assert got == 0


@pytest.mark.parametrize("t", THRESHOLDS)
@pytest.mark.parametrize("field", range(4))
def test_folded_pairs_that_cancel(t, field):
    """differences on both bits of folded pairs are invisible: 48-bit distance t - 1 (flagged) at a 64-bit distance
    beyond the threshold, which the re-check then drops"""
    rng = np.random.default_rng(7 * t + field)
    row = _rand64(rng, 1)[0]
    nd = [_far(rng, row, t) for _ in range(4)]
    vis = min(t - 1, 8)
    nd[field] = M.flip(row, 0, vis, cancel=8)
    assert M.popc48(row, nd[field]) == vis and M.hamm64(row, nd[field]) == vis + 16
    assert M.candidates(M.chain(row, nd, t)) & (1 << field)


@pytest.mark.parametrize("t", THRESHOLDS)
@pytest.mark.parametrize("k", range(3))
def test_borrow_keeps_every_true_match(t, k):
    """field k at h = 48 (the complement: negative, borrows one from field k + 1) beside h = t - 1 and h = t in field
    k + 1: the true match stays flagged, h = t (not a match) may drop out"""
    rng = np.random.default_rng(11 * t + k)
    row = _rand64(rng, 1)[0]
    comp = row ^ 0xFFFF0000FFFFFFFF  # every element of the 48-bit word differs
    assert M.popc48(row, comp) == 48
    for h, must in ((t - 1, True), (t, False)):
        if h > 16:
            continue
        nd = [_far(rng, row, t) for _ in range(4)]
        nd[k], nd[k + 1] = comp, M.flip(row, 1, h)
        got = M.candidates(M.chain(row, nd, t))
        if must:
            assert got & (1 << (k + 1)), (t, k)
        if 48 > 32 + t:  # (at t = 16 the field ends at 0: no borrow, no flag)
            assert got & (1 << k) or got == 0xF  # the wrapped field reads as flagged: a false candidate
        elif k + 1 < 3:  # (below the top field, whose flag makes every field a candidate)
            assert not got & (1 << k) and got & (1 << (k + 1))


@pytest.mark.parametrize("t", THRESHOLDS)
def test_top_field_carry_makes_all_fields_candidates(t):
    rng = np.random.default_rng(13 * t)
    row = _rand64(rng, 1)[0]
    nd = [_far(rng, row, t) for _ in range(3)] + [M.flip(row, 2, t - 1)]
    bits = M.chain(row, nd, t)
    assert bits >> 23 == 151 and M.candidates(bits) == 0xF
    # ... also with the field below it wrapped
    nd[2] = row ^ 0xFFFF0000FFFFFFFF
    assert M.candidates(M.chain(row, nd, t)) == 0xF


def test_random_chains_flag_every_true_match():
    """no construction: near and far needles at random in all four fields; every hamm64 < t is a candidate, and where no
    field wraps the flags are exactly h48 <= t"""
    rng = np.random.default_rng(5)
    for t in THRESHOLDS:
        for _ in range(150):
            row = _rand64(rng, 1)[0]
            nd = []
            for f in range(4):
                kind = int(rng.integers(0, 4))
                if kind == 0:
                    nd.append(_rand64(rng, 1)[0])
                elif kind == 1:
                    nd.append(row ^ 0xFFFF0000FFFFFFFF ^ int(rng.integers(0, 4)))
                else:
                    x = row
                    for i in rng.choice(64, int(rng.integers(0, t + 3)), replace=False).tolist():
                        x ^= 1 << i
                    nd.append(x)
            got = M.candidates(M.chain(row, nd, t))
            h48 = [M.popc48(row, x) for x in nd]
            for f in range(4):
                if M.hamm64(row, nd[f]) < t:
                    assert got & (1 << f), (t, f, h48)
            if max(h48) <= 32 + t and h48[3] > t:
                assert got == sum(1 << f for f in range(3) if h48[f] <= t)
