"""The 16-bit prefilter of the 64-bit matrix-core scan (cbird_amd/csrc/hamm64_mfma.hip, PRE16), restated in numpy.

The word is  f16(x) = fold32(x) ^ (fold32(x) >> 16),  fold32 = lo ^ hi: bit i is the XOR of bits i, i + 16, i + 32, i + 48
of x (fp4_sign.h, fold16).  A set bit of f16(a) ^ f16(b) needs an odd number of set bits among those four of a ^ b, so
popc(f16(a) ^ f16(b)) <= hamm64(a, b).

One accumulator register = one haystack row against FOUR needles P, Q, R, S (the needle tiles of a quadruple, same column)
through ONE 32x32x64 FP4 MFMA.  Every scale block of 32 elements is split by magnitude: sub-block 0 at +-0.5, sub-block 1
at +-4, on both operands.  The haystack holds its word in all four sub-blocks; the needle operand holds P | Q in K block 0
and R | S in K block 1.  A block's sum is  0.25 dot(first) + 16 dot(second),  dot = 16 - 2 d16; the B block scales 2 | 2^13
put the four at 0.5, 32, 2^11, 2^17 = 64^f / 2, so field f (6 bits at bit 6 f) gains 8 - d16_f on the 24 + b that C0 puts
there (b = thresh - 1): 32 + b - d16_f in [16 + b, 32 + b].  Bit 5 of a field <=> d16_f <= b; the top field flags by the
carry into the f32 exponent (bit 23 of the pattern), after which the lower fields are unreadable.

The model follows the hardware as far as the kernel relies on it: the products of one scale block are summed exactly, each
block sum is scaled and added to the float32 accumulator, block by block in order.
"""
import numpy as np

import scan_layout as S

HALF, FOUR = 0.5, 4.0
SCALES = (2.0, 2.0 ** 13)                      # B block scales of K block 0 | 1
WEIGHTS = (0.5, 32.0, 2.0 ** 11, 2.0 ** 17)    # what one element of field f adds: 64^f / 2
FIELD_ONES = 1 + (1 << 6) + (1 << 12) + (1 << 18)
MAX_THRESH = 8                                 # C0 < 2^24 needs 24 + b < 32
ITEM_CAP = 63 + 64 * 8                         # kItemCap
PEND_CAP = 320                                 # kPendCap
QUAD = 128                                     # needles per step


def fold16(x) -> np.ndarray:
    x = np.asarray(x, np.uint64)
    f = (x ^ (x >> np.uint64(32))) & S.M32
    return ((f ^ (f >> np.uint64(16))) & np.uint64(0xFFFF)).astype(np.uint32)


def d16(a, b):
    return np.bitwise_count(fold16(a) ^ fold16(b))


def c0(b: int) -> np.float32:
    """the accumulator's start: every field at 24 + b"""
    return np.float32(2.0 ** 23 + (24 + b) * FIELD_ONES)


def register(d, b: int) -> np.ndarray:
    """f32 bit patterns of accumulators whose four fields meet fold16 distances d[..., 0..3] (arrays), at b = thresh - 1:
    np.float32 adds in the hardware's order -- block sum (exact) first, then the accumulator, K block 0 before 1"""
    d = np.asarray(d, np.float64)
    dot = 16.0 - 2.0 * d
    acc = np.full(d.shape[:-1], c0(b), np.float32)
    for kb in range(2):
        s = (HALF * HALF * dot[..., 2 * kb] + FOUR * FOUR * dot[..., 2 * kb + 1]) * SCALES[kb]  # float64: exact
        acc = (acc + s.astype(np.float32)).astype(np.float32)
    return acc.view(np.uint32)


def _signs(w16: int) -> np.ndarray:
    return np.array([1.0 if (w16 >> i) & 1 else -1.0 for i in range(16)])


def chain(row, needles, b: int) -> int:
    """the same register from the operands themselves: hash `row` against the hashes (P, Q, R, S)"""
    hs = _signs(int(fold16(row)))
    acc = c0(b)
    for kb in range(2):
        s = float(np.dot(hs * HALF, _signs(int(fold16(needles[2 * kb]))) * HALF)
                  + np.dot(hs * FOUR, _signs(int(fold16(needles[2 * kb + 1]))) * FOUR))
        acc = np.float32(acc + np.float32(s * SCALES[kb]))
    return int(np.array([acc], np.float32).view(np.uint32)[0])


def candidates(bits):
    """the fields the kernel re-checks for a register (bit f = field f): all four after a carry into the exponent"""
    bits = np.asarray(bits, np.uint32)
    low = ((bits >> 5) & 1) | (((bits >> 11) & 1) << 1) | (((bits >> 17) & 1) << 2)
    return np.where((bits >> 23) & 1, 0xF, low)


def reference_candidates(hashes, needles, t: int):
    """(i, j) of every (slot, needle) pair the prefilter must hand to the re-check: fold16 distance < t"""
    return S.pairs_below(fold16(hashes), fold16(needles), t)


# ---- the kernel's bookkeeping: descriptors, items (as tests/test_scan_prefilter_items.py restates PRE's) ------------------
def descriptors(hashes, needles, t: int):
    """{(wave, chunk): {step: [cm, ...]}}: one descriptor per hit (group, lane) of a step, cm bit 4 chain + f = field f is
    a candidate in the rows of chain `chain` (registers 0..16 | 17..31 of the group's two tiles).  Padding slots and
    padding needles are hash 0, as in the kernel."""
    n, nq = len(hashes), len(needles)
    n_pairs = S._cdiv(nq, 64)
    qpc = S.prefilter_pairs_per_chunk(n, nq) // 2
    sf = np.zeros(S._cdiv(n, S.WAVE_ROWS) * S.WAVE_ROWS, np.uint32)
    sf[:n] = fold16(hashes)
    nf = np.zeros(S._cdiv(n_pairs, 2) * QUAD, np.uint32)
    nf[:nq] = fold16(needles)
    i, j = S.pairs_below(sf, nf, t)
    Q = j // QUAD
    chunk, step, field = Q // qpc, Q % qpc, (j % QUAD) // 32
    W, rw = i // S.WAVE_ROWS, i % S.WAVE_ROWS
    g, half = S.row_reg(rw % 32)
    lane = (j % 32) + 32 * half
    ch = (16 * ((rw // 32) % 2) + g > 16).astype(np.int64)
    flags = {}
    for k in zip(W.tolist(), chunk.tolist(), step.tolist(), (rw // 64).tolist(), lane.tolist(), ch.tolist(), field.tolist()):
        flags[k[:5]] = flags.get(k[:5], 0) | (1 << (4 * k[5] + k[6]))
    out = {}
    for (w, c, s, gr, ln), bb in sorted(flags.items()):
        cm = sum((0xF if (bb >> (4 * x)) & 8 else (bb >> (4 * x)) & 7) << (4 * x) for x in (0, 1))
        out.setdefault((w, c), {}).setdefault(s, []).append(cm)
    return out


def trace(hashes, needles, t: int):
    """per wave instance: the most descriptors and items its lists held, what every non-final drain kept"""
    res = {}
    for inst, steps in descriptors(hashes, needles, t).items():
        tr = {"pend_peak": 0, "item_peak": 0, "kept_desc": [], "kept_items": [], "items": 0}
        pend, nitem = [], 0

        def drain(final):
            nonlocal pend, nitem
            keep = 0 if final else len(pend) & 63
            k0 = keep
            while True:
                if nitem < 64 and k0 < len(pend):
                    c = sum(int(cm).bit_count() for cm in pend[k0:k0 + 64])
                    nitem += c
                    tr["items"] += c
                    tr["item_peak"] = max(tr["item_peak"], nitem)
                    k0 += 64
                elif nitem >= 64:
                    nitem -= 64
                elif final and nitem:
                    nitem = 0
                else:
                    break
            pend = pend[:keep]
            if not final:
                tr["kept_desc"].append(keep)
                tr["kept_items"].append(nitem)

        for s in sorted(steps):
            pend += steps[s]
            tr["pend_peak"] = max(tr["pend_peak"], len(pend))
            if len(pend) >= 64:
                drain(False)
        drain(True)
        res[inst] = tr
    return res


def row_chain(rw: int) -> int:
    """reduction chain (0 | 1) of wave row rw"""
    g, _ = S.row_reg(rw % 32)
    return int(16 * ((rw // 32) % 2) + int(g) > 16)


def kernel_word(rng, k: int) -> np.ndarray:
    """k random u64 with fold16 = 0: every column i has an even number of set bits among i, i + 16, i + 32, i + 48"""
    even = np.array([0b0000, 0b0011, 0b0101, 0b0110, 0b1001, 0b1010, 0b1100, 0b1111], np.uint64)
    out = np.zeros(k, np.uint64)
    for i in range(16):
        p = even[rng.integers(0, 8, k)]
        for r in range(4):
            out |= ((p >> np.uint64(r)) & np.uint64(1)) << np.uint64(i + 16 * r)
    return out
