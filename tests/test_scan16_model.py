"""The 16-bit prefilter's arithmetic on paper (tests/scan16_layout.py; k_hamm64_mfma16 in cbird_amd/csrc/hamm64_mfma.hip):
one f32 accumulator register for every combination of four fold16 distances at every threshold the kernel serves, and the
lower bound the prefilter rests on.  No GPU."""
import functools
import os
import sys

import numpy as np
import pytest

import scan16_layout as M
import scan_layout as S


@functools.lru_cache(maxsize=None)
def _all_distances():
    d = np.arange(17)
    return np.stack(np.meshgrid(d, d, d, d, indexing="ij"), axis=-1).reshape(-1, 4)  # 83 521 x (d0, d1, d2, d3)


def test_weights_are_one_field_apart():
    """0.5 x 0.5 and 4 x 4 under the block scales 2 | 2^13: 64^f / 2 per element of field f"""
    got = [M.HALF * M.HALF * M.SCALES[0], M.FOUR * M.FOUR * M.SCALES[0], M.HALF * M.HALF * M.SCALES[1],
           M.FOUR * M.FOUR * M.SCALES[1]]
    assert got == list(M.WEIGHTS) == [64.0 ** f / 2 for f in range(4)]
    for b in range(M.MAX_THRESH):
        assert float(M.c0(b)) == 2.0 ** 23 + (24 + b) * M.FIELD_ONES < 2.0 ** 24
    assert 2.0 ** 23 + (24 + M.MAX_THRESH) * M.FIELD_ONES >= 2.0 ** 24  # threshold 9 does not fit


@pytest.mark.parametrize("b", range(M.MAX_THRESH))
def test_every_register(b):
    """every (d0, d1, d2, d3) in [0, 16]^4: the flag bits are exactly d_f <= b, or bit 23 when the top field flags; no
    accumulator below the carry leaves [2^23, 2^24) and its fields read 32 + b - d_f"""
    d = _all_distances()
    bits = M.register(d, b)
    top = d[:, 3] <= b
    carried = ((bits >> 23) & 1).astype(bool)
    assert np.array_equal(carried, top)
    val = bits.view(np.float32)
    assert (val[~top] >= np.float32(2.0 ** 23)).all() and (val[~top] < np.float32(2.0 ** 24)).all()
    assert (val[top] >= np.float32(2.0 ** 24)).all() and (val[top] < np.float32(2.0 ** 25)).all()  # one carry, no more
    lo = bits[~top]
    for f in range(4):
        field = (lo >> (6 * f)) & 63
        assert np.array_equal(field, (32 + b - d[~top, f]).astype(np.uint32)), f
        if f < 3:
            assert np.array_equal(((lo >> (6 * f + 5)) & 1).astype(bool), d[~top, f] <= b), f
    assert ((lo >> 24) == (0x4B000000 >> 24)).all()
    # what the kernel re-checks: never fewer fields than are under the threshold
    under = sum(((d[:, f] <= b).astype(np.uint32) << f) for f in range(4))
    cand = M.candidates(bits)
    assert ((cand & under) == under).all()
    assert np.array_equal(cand[~top], under[~top]) and (cand[top] == 0xF).all()


def test_registers_from_the_operands():
    """the sign vectors themselves through the two block sums give the register the distance formula gives"""
    rng = np.random.default_rng(5)
    for k in range(200):
        row = S._rand64(rng, 1)[0]
        needles = S._rand64(rng, 4)
        for f in range(4):  # near words, so that fields flag
            if rng.integers(0, 2):
                needles[f] = S._near(rng, row, 1, 6)[0]
        b = int(rng.integers(0, M.MAX_THRESH))
        d = np.array([int(M.d16(row, x)) for x in needles])
        assert M.chain(row, needles, b) == int(M.register(d[None, :], b)[0]), k


def _bound(a, b):
    assert (M.d16(a, b) <= np.bitwise_count(a ^ b)).all()


def test_fold16_is_a_lower_bound_on_random_pairs():
    rng = np.random.default_rng(6)
    a = S._rand64(rng, 1_000_000)
    _bound(a, S._rand64(rng, 1_000_000))
    near = a.copy()  # and on near pairs, where the bound is tight or cancels
    for _ in range(6):
        near ^= np.uint64(1) << rng.integers(0, 64, len(a), dtype=np.uint64)
    _bound(a, near)
    w = M.kernel_word(rng, 4096)
    assert (M.fold16(w) == 0).all() and (M.d16(a[:4096], a[:4096] ^ w) == 0).all()


def test_fold16_is_a_lower_bound_on_image_hashes(orc):
    """the 17 997 000 pairs of 6000 benchmark images (bench.gen_images, seed 1234) hashed on the CPU by oracle/fast_hash.c
    -- tests/golden/bench_hashes_6000_seed1234.npy; the last 64 are made again here.  Their fold16 candidate rate at
    threshold 1 is that of uniform 16-bit words, 2^-16 = 1.53e-5 per pair, true matches apart"""
    import torch

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    try:
        import bench
    finally:
        sys.path.pop(0)
    n = 6000
    h = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bench_hashes_6000_seed1234.npy"))
    assert h.dtype == np.uint64 and len(h) == n
    again = orc.dcthash64_fast256_batch(bench.gen_images(torch, "cpu", n - 64, n, n, 1234).numpy())
    assert np.array_equal(again, h[n - 64:])
    false1 = 0
    for i0 in range(0, n, 500):
        x = h[i0:i0 + 500, None] ^ h[None, :]
        d64 = np.bitwise_count(x)
        dd = M.d16(h[i0:i0 + 500, None], h[None, :])
        assert (dd <= d64).all()
        upper = np.arange(n)[None, :] > np.arange(i0, min(n, i0 + 500))[:, None]
        false1 += int(((dd < 1) & (d64 >= 1) & upper).sum())
    pairs = n * (n - 1) // 2
    assert pairs == 17_997_000
    assert 1.0e-5 < false1 / pairs < 2.2e-5, false1 / pairs


def test_reference_candidates_hold_every_true_match():
    rng = np.random.default_rng(7)
    slots, needles = S._rand64(rng, 512), S._rand64(rng, 256)
    needles[::3] = S._near(rng, slots[5], len(needles[::3]), 9)
    for t in (1, 2, 4, 8):
        i, j = M.reference_candidates(slots, needles, t)
        have = set(zip(i.tolist(), j.tolist()))
        ti, tj = S.pairs_below(slots, needles, t)
        assert set(zip(ti.tolist(), tj.tolist())) <= have
