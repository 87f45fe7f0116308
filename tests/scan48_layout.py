"""The 48-bit prefilter of the 64-bit matrix-core scan (cbird_amd/csrc/hamm64_mfma.hip, PRE48), restated in numpy.

One chain = one haystack row against FOUR needles P, Q, R, S through three chained 32x32x64 FP4 MFMAs into one f32
accumulator.  The prefilter word has three sub-blocks of 16 elements (fp4_sign.h, pre48_sub):
    E0 = (lo ^ hi) & 0xffff   the folds  bit i ^ bit i + 32,  i < 16
    E1 = lo >> 16             bits 16..31 as they are
    E2 = hi >> 16             bits 48..63 as they are
The haystack lanes of K block 0 hold Y = (E0, E1, E2, E0 x 8), those of K block 1 hold X = (E2, E0 x 8, E1, E2), every
element +-0.5 except the "x 8" sub-blocks at +-4; MFMA m reads sub-blocks m, m + 1 of both.  The needle side is the twelve
sub-blocks P.E0 P.E1 P.E2 Q.E0 ... S.E2 in a row, two per K block, at +-0.5 except Q.E0, R.E1 and S.E0 at +-4.  The block
scales 2 | 2, 2^7 | 2^10, 2^13 | 2^19 give every element of field f the weight 64^f / 2, so field f gains 24 - h_f.

The model follows the hardware as far as the kernel relies on it: the products of one scale block are summed exactly
(float64 here), each block sum is scaled and added to the float32 accumulator, block by block in order.
"""
import numpy as np

HALF, FOUR = 0.5, 4.0
HAY = (((0, HALF), (1, HALF), (2, HALF), (0, FOUR)),   # Y: the lanes of K block 0
       ((2, HALF), (0, FOUR), (1, HALF), (2, HALF)))   # X: the lanes of K block 1
NEEDLE_FOUR = (3, 7, 9)                                # needle sub-blocks (of 12) at magnitude 4: Q.E0, R.E1, S.E0
SCALES = ((2.0, 2.0), (2.0 ** 7, 2.0 ** 10), (2.0 ** 13, 2.0 ** 19))
FIELD_ONES = 1 + (1 << 6) + (1 << 12) + (1 << 18)
MAX_THRESH = 16


def sub(h, k):
    """sub-block k (16 bits) of the prefilter word of hash h"""
    h = int(h)
    lo, hi = h & 0xFFFFFFFF, h >> 32
    return ((lo ^ hi) & 0xFFFF, lo >> 16, hi >> 16)[k]


def word48(h):
    return sub(h, 0) | (sub(h, 1) << 16) | (sub(h, 2) << 32)


def popc48(a, b):
    return bin(word48(a) ^ word48(b)).count("1")


def hamm64(a, b):
    return bin(int(a) ^ int(b)).count("1")


def _signs(w16):
    return np.array([1.0 if (w16 >> i) & 1 else -1.0 for i in range(16)])


def c0(t):
    """the accumulator's start: every field at 8 + t, so that it ends at 32 + t - h"""
    return np.float32(2.0 ** 23 + (8 + t) * FIELD_ONES)


def chain(row, needles, t):
    """the f32 bit pattern one accumulator register ends with: `row` against needles (P, Q, R, S) at threshold t"""
    acc = c0(t)
    for m in range(3):
        for kb in range(2):
            s = 0.0  # float64: the block sum is exact
            for j in range(2):
                e, mag = HAY[kb][m + j]
                slot = 2 * (2 * m + kb) + j
                nmag = FOUR if slot in NEEDLE_FOUR else HALF
                s += float(np.dot(_signs(sub(row, e)) * mag, _signs(sub(needles[slot // 3], slot % 3)) * nmag))
            acc = np.float32(acc + np.float32(s * SCALES[m][kb]))
    return int(np.array([acc], np.float32).view(np.uint32)[0])


def candidates(bits):
    """the fields the kernel re-checks for this register: bit f = field f.  A carry into the exponent (the top field's
    flag) leaves the lower fields unreadable: all four are candidates."""
    if (bits >> 23) & 1:
        return 0xF
    return ((bits >> 5) & 1) | (((bits >> 11) & 1) << 1) | (((bits >> 17) & 1) << 2)


def fields(bits):
    """the four 6-bit fields (meaningful while the exponent has not moved)"""
    return [(bits >> (6 * f)) & 63 for f in range(4)]


def flip(h, sub_block, count, cancel=0):
    """h with `count` elements of sub-block k flipped (k = 0: one bit of each of `count` folded pairs) and, for k = 0,
    BOTH bits of `cancel` further folded pairs -- those cancel in the fold"""
    h = int(h)
    if sub_block == 0:
        for i in range(count):
            h ^= 1 << i
        for i in range(count, count + cancel):
            h ^= (1 << i) | (1 << (i + 32))
    else:
        base = 16 if sub_block == 1 else 48
        for i in range(count):
            h ^= 1 << (base + i)
    return h
