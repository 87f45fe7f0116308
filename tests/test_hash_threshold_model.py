"""tests/hash_threshold_cases.py on the CPU: the builders deliver what they promise, every lifted image really has its
target tile, and -- the point of the exercise -- tiles built this way DO notice a changed rounding where random tiles do
not: the repository's own oracle sources recompiled with -ffp-contract=fast, and the oracle's other evaluation of the
same transform (variant 0), change a large share of the constructed hashes and next to none of 20 000 random ones."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hash_threshold_cases as H

SEED = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_impulse_responses_are_the_float64_oracles(orc):
    """G[k] is the exact response of coef[k] - thr to +1 on a pixel: the float64 evaluation moves by it"""
    G = H.impulse_responses()
    rng = np.random.default_rng(5)
    tile = H.family_tiles(rng, 1)[0]
    _, c0, t0 = orc.hash_from_tile32_v(tile, 2, with_coefs=True)
    for _ in range(20):
        r, c = (int(v) for v in rng.integers(0, 32, 2))
        t = tile.copy()
        t[r, c] += 1
        _, c1, t1 = orc.hash_from_tile32_v(t, 2, with_coefs=True)
        assert np.abs(((c1 - t1) - (c0 - t0)) - G[:, r, c]).max() < 1e-10
    assert np.abs((c0 - t0) - G.reshape(64, -1) @ tile.reshape(-1).astype(np.float64)).max() < 1e-9


def test_ordered_int_is_float_order():
    x = np.float32(3.25)
    up, down = np.nextafter(x, np.float32(9)), np.nextafter(x, np.float32(0))
    assert H.ordered_int(up) - H.ordered_int(x) == 1 and H.ordered_int(down) - H.ordered_int(x) == -1
    tiny = np.nextafter(np.float32(0), np.float32(1))
    assert H.ordered_int(tiny) == 1 and H.ordered_int(-tiny) == -1 and H.ordered_int(np.float32(-0.0)) == 0
    assert H.ordered_int(np.float32(-3.25)) == -H.ordered_int(x)


def test_near_threshold_tiles_meet_their_conditions(orc):
    cases = H.near_threshold_tiles(SEED)
    assert sorted(c.bit for c in cases) == list(range(1, 64))
    for c in cases:
        assert c.tile.dtype == np.uint8 and c.tile.shape == (32, 32)
        assert H.PIX_LO <= int(c.tile.min()) and int(c.tile.max()) <= H.PIX_HI
        h, co, thr = orc.hash_from_tile32_v(c.tile, 1, with_coefs=True)
        thr = np.float32(thr)
        assert H.ordered_int(co[c.bit]) - H.ordered_int(thr) == c.rel and abs(c.rel) <= 1
        assert h == c.hash and ((h >> c.bit) & 1) == (1 if c.rel > 0 else 0)
        assert (co[1:] > thr).any()  # no tile is hashed by the 0 -> 1 rule
        assert orc.hash_from_tile32(c.tile) == h  # (variant 1 is the oracle's default)
    for rel in (0, 1, -1):
        assert sum(c.rel == rel for c in cases) >= 8, rel


def test_builders_are_seeded():
    a = H.near_threshold_tiles.__wrapped__(SEED)
    b = H.near_threshold_tiles(SEED)
    assert [(x.bit, x.rel, x.hash, x.tile.tobytes()) for x in a] == [(x.bit, x.rel, x.hash, x.tile.tobytes()) for x in b]
    other = H.near_threshold_tiles(SEED + 1)
    assert any(x.tile.tobytes() != y.tile.tobytes() for x, y in zip(a, other))
    for c in (a[0], a[31], a[62]):
        x, y = H.lift_to_256(c, SEED), H.lift_to_256(c, SEED)
        assert x is not None and x.tobytes() == y.tobytes()
    k1, k2 = H.kp_square_case.__wrapped__(SEED), H.kp_square_case(SEED)
    assert len(k1) == len(k2) and all(p.image.tobytes() == q.image.tobytes() for p, q in zip(k1, k2))


def test_lifted_images_have_exactly_their_tiles(orc):
    cases, imgs, failed = H.lifted_cases(SEED)
    assert len(cases) >= 48 and len(cases) + len(failed) == 63, failed
    assert sorted([c.bit for c in cases] + failed) == list(range(1, 64))  # what did not lift is named, not dropped
    assert imgs.shape == (len(cases), 256, 256) and imgs.dtype == np.uint8
    for c, im in zip(cases, imgs):
        assert (orc.tile32(im) == c.tile).all(), c.bit
        assert c.hash == orc.hash_from_tile32_v(c.tile, 1)
    want = np.array([c.hash for c in cases], np.uint64)
    assert (orc.dcthash64_batch(imgs) == want).all()
    assert (orc.dcthash64_fast256_batch(imgs) == want).all()
    for rel in (0, 1, -1):
        assert sum(c.rel == rel for c in cases) >= 8, rel


def test_keypoint_square_cases(orc):
    cases = H.kp_square_case(SEED)
    assert len(cases) >= 6
    for c in cases:
        assert c.image.shape == (300, 300) and abs(c.rel) <= 1
        got, blurred = orc.keypoint_hashes(c.image, c.kp)
        assert len(got) == 1 and int(got[0]) == c.hash == orc.hash_from_tile32_v(c.tile, 1)
        x0, y0 = int(c.kp[0, 0]), int(c.kp[0, 1])
        sums = blurred[y0:y0 + 256, x0:x0 + 256].astype(np.int64).reshape(32, 8, 32, 8).sum(axis=(1, 3))
        assert (np.rint(sums / 64.0) == c.tile).all()
        assert H.coef_thr_distance(orc, c.tile, c.bit)[0] == c.rel
    assert {c.rel for c in cases} == {0, 1, -1}


def _contracted_oracle(tmp_path):
    """libcbird_oracle.so from the repository's oracle sources by its own Makefile, -ffp-contract=fast in place of off"""
    if not (shutil.which("make") and shutil.which(os.environ.get("CC", "gcc")) and shutil.which("g++")):
        pytest.skip("no compiler here")
    src = os.path.join(ROOT, "oracle")
    for f in os.listdir(src):
        if f.endswith(".c") or f in ("retain_stl.cpp", "Makefile"):
            shutil.copy(os.path.join(src, f), tmp_path / f)
    with open(os.path.join(src, "Makefile")) as fh:
        flags = re.search(r"^CFLAGS = (.*)$", fh.read(), re.M).group(1)
    assert "-ffp-contract=off" in flags
    subprocess.check_call(["make", "-C", str(tmp_path), "libcbird_oracle.so",
                           "CFLAGS=" + flags.replace("-ffp-contract=off", "-ffp-contract=fast")],
                          stdout=subprocess.DEVNULL)
    L = C.CDLL(str(tmp_path / "libcbird_oracle.so"))
    L.orc_hash_tiles_stats.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    L.orc_hash_tiles_stats.restype = None
    return L


def test_constructed_tiles_notice_a_changed_rounding_random_ones_do_not(orc, tmp_path, capsys):
    """Sensitivity is measured, not assumed.  Against the oracle as built (variant 1):
      (a) the same sources with contracted multiply-adds, variant 1;
      (b) the oracle's canonical evaluation of the same transform (variant 0).
    Each must change at least 10 of the constructed hashes, at a rate at least 1000 times the rate over 20 000 random
    tiles of the family the constructed ones come from (no random flip counts as one)."""
    L = _contracted_oracle(tmp_path)
    built = np.stack([c.tile for c in H.near_threshold_tiles(SEED)] + [c.tile for c in H.kp_square_case(SEED)])
    rnd = H.family_tiles(np.random.default_rng(2024), 20000)

    def contracted(tiles):
        tiles = np.ascontiguousarray(tiles)
        hs = np.zeros(len(tiles), np.uint64)
        L.orc_hash_tiles_stats(tiles.ctypes.data, len(tiles), 1, hs.ctypes.data, None)
        return hs

    ref_built, ref_rnd = orc.hash_tiles_stats(built, 1)[0], orc.hash_tiles_stats(rnd, 1)[0]
    assert ref_built.tolist() == [orc.hash_from_tile32_v(t, 1) for t in built]
    for name, hb, hr in (("-ffp-contract=fast", contracted(built), contracted(rnd)),
                         ("variant 0", orc.hash_tiles_stats(built, 0)[0], orc.hash_tiles_stats(rnd, 0)[0])):
        nb, nr = int((hb != ref_built).sum()), int((hr != ref_rnd).sum())
        with capsys.disabled():
            print(f"\n[hash threshold] {name}: {nb} of {len(built)} constructed hashes change, {nr} of {len(rnd)} random")
        assert nb >= 10, (name, nb)
        assert nb / len(built) >= 1000 * max(nr, 1) / len(rnd), (name, nb, nr)
