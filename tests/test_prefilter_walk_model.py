"""The prefilter drain's two-stage row walk (`work` in prefilter_body, cbird_amd/csrc/hamm64_mfma.hip) on paper.  CPU only.

Stage 1 looks at the 32-bit fold of every row of an item's chain: three instructions per row,
    x = lo ^ hi ^ fold(needle)                 (one three-input xor)
    s = popc(x) + (2^31 - thresh)              (v_bcnt_u32_b32 with its add operand preloaded)
    far = (far << 1) | (s >> 31)               (v_alignbit_b32 of far : s by 31)
with the rows fed from the chain's last to its first, so that row k ends in bit k of `far`.  Stage 2 re-checks the rows
whose bit is clear on all 64 bits.  Checked here: the arithmetic of the preloaded constant, the bit order against cd_row,
and that the fold distance never exceeds the 64-bit distance -- for whichever prefilter word raised the flag."""
import numpy as np

import scan16_layout as M
import scan_layout as S

U32 = np.uint64(0xFFFFFFFF)


def alignbit(hi, lo, shift):
    """v_alignbit_b32: the low 32 bits of (hi : lo) >> shift"""
    return int(((np.uint64(hi) << np.uint64(32) | np.uint64(lo)) >> np.uint64(shift)) & U32)


def far_bit(popc, thresh):
    """bit 31 of the v_bcnt_u32_b32 sum, in 32-bit arithmetic"""
    return ((popc + ((1 << 31) - thresh)) & 0xFFFFFFFF) >> 31


def chain_rows(ch):
    """registers of chain `ch` by mask bit k = register 16 ch + k: 17 valid bits, then 15"""
    return {k: 16 * ch + k for k in (range(17) if ch == 0 else range(1, 16))}


def walk(rows_lo_hi, qfold, thresh, order):
    """`far` after feeding rows (lo, hi) in `order` through the three instructions"""
    far = 0
    for k in order:
        lo, hi = rows_lo_hi[k]
        s = (int(np.bitwise_count(np.uint32(lo ^ hi ^ qfold))) + ((1 << 31) - thresh)) & 0xFFFFFFFF
        far = alignbit(far, s, 31)
    return far


def test_preloaded_constant_puts_popc_ge_thresh_in_bit_31():
    for thresh in range(1, 33):
        for popc in range(0, 33):
            assert far_bit(popc, thresh) == (1 if popc >= thresh else 0), (popc, thresh)
            assert popc + ((1 << 31) - thresh) < (1 << 32)  # the sum never wraps


def test_alignbit_by_31_shifts_in_from_below():
    assert alignbit(0, 0x80000000, 31) == 1 and alignbit(0, 0x7FFFFFFF, 31) == 0
    assert alignbit(0b101, 0x80000000, 31) == 0b1011 and alignbit(0b101, 0x00000010, 31) == 0b1010
    assert alignbit(0xFFFFFFFF, 0, 31) == 0xFFFFFFFE  # what falls off the top is gone


def test_mask_bit_k_is_register_16c_plus_k():
    """the kernel feeds the chain's fifth-quad row first (hq[32]: register 16 for chain 0; chain 1 reads its row 0 there
    and masks it), then quads 3..0 with rows 3..0: seventeen shift-ins, row k in bit k; hq[k + (k & 0x1c)] is that row"""
    rng = np.random.default_rng(5)
    for ch in (0, 1):
        valid = chain_rows(ch)
        assert len(valid) == (17, 15)[ch]
        assert sum(1 << k for k in valid) == (0x1FFFF, 0xFFFE)[ch]  # `rows` in the kernel
        for half in (0, 1):
            for k, reg in valid.items():
                # hq = the wave row of register 16 ch; row k of the chain sits 8 (k >> 2) + (k & 3) rows on
                want = 32 * (reg >> 4) + S.reg_row(reg & 15, half)
                base = 32 * ch + S.reg_row(0, half)
                assert base + k + (k & 0x1C) == want == base + 8 * (k >> 2) + (k & 3), (ch, half, k)
        for thresh in (1, 2, 7, 16):
            q = int(rng.integers(0, 1 << 32))
            rows = {}
            for k in range(17):
                d = int(rng.integers(0, 2 * thresh + 1))
                x = sum(1 << int(b) for b in rng.choice(32, min(d, 32), replace=False))
                lo = int(rng.integers(0, 1 << 32))
                rows[k] = (lo, lo ^ q ^ x)  # fold(row) ^ q = x: fold distance popc(x)
            order = [16 if ch == 0 else 0] + [4 * i + j for i in (3, 2, 1, 0) for j in (3, 2, 1, 0)]
            far = walk(rows, q, thresh, order)
            assert far < (1 << 17)
            survivors = ~far & (0x1FFFF, 0xFFFE)[ch]
            for k in valid:
                d = int(np.bitwise_count(np.uint32(rows[k][0] ^ rows[k][1] ^ q)))
                assert bool((survivors >> k) & 1) == (d < thresh), (ch, thresh, k, d)
            if ch == 1:
                assert not survivors & 1 and not survivors >> 16


def test_fold_distance_bounds_the_64_bit_distance():
    rng = np.random.default_rng(6)
    a = S._rand64(rng, 4096)
    b = a.copy()
    for i in range(len(b)):  # near neighbours: 0..12 flipped bits, collisions i | i + 32 among them
        for bit in rng.choice(64, int(rng.integers(0, 13)), replace=False):
            b[i] ^= np.uint64(1) << np.uint64(int(bit))
    b[::7] = S._rand64(rng, len(b[::7]))
    d64 = np.bitwise_count(a ^ b)
    dfold = np.bitwise_count(S.fold(a) ^ S.fold(b))
    assert (dfold <= d64).all() and ((d64 - dfold) % 2 == 0).all()
    for thresh in range(1, 33):
        assert (dfold[d64 < thresh] < thresh).all()
    # ... and whichever word raised the flag: the 16-bit fold is a fold of the 32-bit one
    assert (M.d16(a, b) <= dfold).all()
    assert (d64 != dfold).any() and (d64 == dfold).any()


def test_flag_gather_multiply():
    """drain: the four flags of a chain, six bits apart (bits 0, 6, 12, 18 after the shift), times 1 + 2^5 + 2^10 + 2^15
    land on bits 15..18 with no other partial product on or carrying into them"""
    for nb in range(16):
        w = sum(((nb >> f) & 1) << (6 * f) for f in range(4))
        assert w < (1 << 24) and 0x8421 < (1 << 24)  # a 24-bit multiply
        assert ((w * 0x8421) >> 15) & 0xF == nb
    for e in np.random.default_rng(7).integers(0, 1 << 32, 2000).tolist():
        for c in (0, 1):
            w = (e >> (5 + c)) & 0x41041
            want = sum(((e >> (5 + c + 6 * f)) & 1) << f for f in range(4))
            assert (((w * 0x8421) & 0xFFFFFFFF) >> 15) & 0xF == want
