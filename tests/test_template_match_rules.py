"""CPU: the numpy model of tests/template_match_rules.py (estimateRigidTransform, the roi, invertAffineTransform +
warpAffine as recalled from OpenCV 2.4.13 -- unpinned) checked against things that do not share its code, and the
conditions on the fixtures that the GPU tests of tests/test_template_match.py rely on.

Measured here (test_fixture_margins prints them): the largest difference between the model's Jacobi and
numpy.linalg.solve over the final solves of the estimate fixture is 3.1e-15, so the matrix tolerance is 16 x that =
4.97e-14; the smallest residual margin of the fixture is 1.0e-3 px ("mirrored"; 0.02 px and more elsewhere) against the
required 1e6 x tolerance = 5.0e-8; the chain's rounding margins are 2.4e-3 .. 7.1e-3 against the required
1e6 x tolerance x 1024 x 40 = 2.04e-3."""
import math

import numpy as np
import pytest

import template_match_rules as R


def test_rng_first_values_by_hand():
    s = 0xFFFFFFFFFFFFFFFF
    want = []
    for _ in range(4):
        s = ((s & 0xFFFFFFFF) * 4164903690 + (s >> 32)) % (1 << 64)
        want.append(s % (1 << 32))
    # the first one worked out on paper: (2^32 - 1) * 4164903690 + (2^32 - 1) = (2^32 - 1) * 4164903691 = -4164903691 mod 2^32
    assert want[0] == (1 << 32) - 4164903691 == 130063605
    r = R.RNG()
    assert [r.next() for _ in range(4)] == want and r.draws == 4
    r = R.RNG()
    assert r.uniform(1000) == 130063605 % 1000


@pytest.mark.parametrize("deg,scale", [(0, 0.5), (30, 1.4), (90, 0.5), (180, 1.4)])
def test_planted_similarity_is_recovered(deg, scale):
    m = R.similarity(deg, scale, 31.5, -12.25)
    a, b = R.planted(np.random.default_rng(5), 300, 210, m, (400.0, 300.0), (200.0, 150.0))
    r = R.estimate_rigid(a, b)
    assert r["found"] and r["good_count"] >= 210 and r["iterations"] <= 60
    assert np.abs(r["m"] - m).max() < 0.2 and np.abs(r["m"][[0, 1, 3, 4]] - m[[0, 1, 3, 4]]).max() < 2e-3
    assert r["m"][0] == r["m"][4] and r["m"][1] == -r["m"][3]


def test_final_fit_agrees_with_least_squares_on_the_design_matrix():
    """numpy.linalg.lstsq on the 2k x 4 design matrix of the inliers never forms the normal equations; the float32
    products in the model's sums allow 1e-4"""
    for name, r in R.estimate_yardstick().items():
        if not r["found"]:
            continue
        a, b = (v.astype(np.float64) for v in R.estimate_fixture()[name])
        g = r["good"]
        one, zero = np.ones(len(g)), np.zeros(len(g))
        A = np.zeros((2 * len(g), 4))
        A[0::2] = np.stack([a[g, 0], -a[g, 1], one, zero], 1)
        A[1::2] = np.stack([a[g, 1], a[g, 0], zero, one], 1)
        x = np.linalg.lstsq(A, b[g].reshape(-1), rcond=None)[0]
        assert np.abs(R.rt_from_x(x) - r["m"]).max() < 1e-4, name


def test_jacobi_solves_the_normal_equations():
    rng = np.random.default_rng(3)
    for _ in range(50):
        a = rng.uniform(-300, 300, (40, 2)).astype(np.float32)
        b = R.apply(R.similarity(rng.uniform(0, 360), rng.uniform(0.3, 2), *rng.uniform(-50, 50, 2)), a).astype(np.float32)
        sa, sb = R.normal_equations(*R.normal_sums(a, b))
        x = R.jacobi_solve(sa, sb)
        assert np.abs(np.array(sa) @ np.array(x) - np.array(sb)).max() <= 1e-9 * np.abs(sb).max()


def test_no_transform_cases():
    y = R.estimate_yardstick()
    for name in R.NOT_FOUND:
        assert not y[name]["found"] and not y[name]["m"].any(), name
    assert [c[0] for c in R.ESTIMATE_CASES if not y[c[0]]["found"]] == list(R.NOT_FOUND)
    assert y["n0"]["iterations"] == y["n2"]["iterations"] == 0 and y["n0"]["draws"] == 0
    assert y["n40_30"]["iterations"] == 500 and y["mirrored"]["iterations"] == 500
    # every inner loop of the second / third draw runs out: 1 + 500 and 2 + 500 draws per outer iteration
    assert y["same_a"]["draws"] == 500 * 501 and y["collinear"]["draws"] >= 500 * 502
    assert y["n3"]["good_count"] == 3 and y["n1000_50"]["good_count"] >= 500 and y["n63"]["found"] and y["n65"]["found"]


def test_fixture_margins():
    """the conditions the GPU comparison rests on, for the model alone: every case's residual margin is at least 1e6 x the
    matrix tolerance, none left out"""
    tol, worst = R.m_tolerance()
    y = R.estimate_yardstick()
    print("largest Jacobi - LU difference", worst, "tolerance", tol)
    assert 0 < tol < 1e-12
    for name, r in y.items():
        print(name, "residual margin", r["residual_margin"], "half margin", r["half_margin"])
        assert r["residual_margin"] >= 1e6 * tol, name


def oracle_score():
    import oracle

    return oracle.PrestageOracle().template_score


def chain_yardstick():
    if "chain_yard" not in R._cache:
        tmpl, cands, al, bl, scales = R.chain_fixture()
        score = oracle_score()
        R._cache["chain_yard"] = [R.template_match(tmpl, [c], a, [b], [s], score)[0]
                                  for c, a, b, s in zip(cands, al, bl, scales)]
    return R._cache["chain_yard"]


def test_chain_fixture_margins():
    """two of six without a transform; the model's rounding margin (coordinate tables and roi quotients) of every other
    candidate is at least 1e6 x tolerance x 1024 x the largest coordinate"""
    tol, _ = R.m_tolerance()
    bound = 1e6 * tol * 1024 * max(R.CHAIN_TW, R.CHAIN_TH)
    y = chain_yardstick()
    assert [r["found"] for r in y] == [True, True, False, True, False, True]
    assert sorted(set(float(s) for s in R.chain_fixture()[4])) == [np.float32(0.37), 1.0]
    for i, r in enumerate(y):
        print(i, "rounding margin", r["rounding_margin"], "bound", bound, "residual margin", r["residual_margin"])
        assert r["residual_margin"] >= 1e6 * tol, i
        if r["found"]:
            assert r["rounding_margin"] >= bound and r["tx_found"] and r["score"] <= 4, i
        else:
            assert r["score"] == R.INT32_MAX and not r["patch"].any()


# ---- the warp against plain array slicing ------------------------------------------------------------------------------
def image(seed, h, w, ch):
    a = np.random.default_rng(seed).integers(1, 256, (h, w, ch), dtype=np.uint8)
    return a[..., 0] if ch == 1 else a


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_warp_identity_and_integer_shifts(ch):
    img = image(ch, 23, 37, ch)
    p, _ = R.warp_affine(img, R.similarity(0, 1, 0, 0), 37, 23)
    assert (p == img).all()
    border = np.array(R.BORDER[ch], np.uint8)
    for dx, dy in ((5, 3), (-4, 2), (6, -7), (-3, -2)):
        # m maps template -> candidate: patch(x, y) = img(x + dx, y + dy)
        p, _ = R.warp_affine(img, R.similarity(0, 1, dx, dy), 37, 23)
        want = np.empty((23, 37, ch), np.uint8)
        want[:] = border
        ys, xs = np.arange(23) + dy, np.arange(37) + dx
        oky, okx = (ys >= 0) & (ys < 23), (xs >= 0) & (xs < 37)
        want[np.ix_(oky, okx)] = img.reshape(23, 37, ch)[np.ix_(ys[oky], xs[okx])]
        assert (p.reshape(23, 37, ch) == want).all(), (dx, dy)


def test_warp_quarter_turn():
    img = image(9, 30, 30, 3)
    # template (x, y) -> candidate (29 - y, x): a 90 degree rotation about the image centre
    p, _ = R.warp_affine(img, np.array([0.0, -1.0, 29.0, 1.0, 0.0, 0.0]), 30, 30)
    want = np.empty_like(img)
    for y in range(30):
        for x in range(30):
            want[y, x] = img[x, 29 - y]
    assert (p == want).all()


def test_warp_outside_and_beyond_the_domain():
    img = image(2, 20, 20, 4)
    p, _ = R.warp_affine(img, R.similarity(0, 1, 500, 500), 16, 16)
    assert (p[..., :3] == 0).all() and (p[..., 3] == 255).all()
    p, _ = R.warp_affine(img, R.similarity(0, 1, 2.0e6, 0), 16, 16)
    assert p is None
    assert R.warp_affine(img, np.zeros(6), 16, 16)[0] is not None  # a singular matrix: D = 0, every tap at (0, 0)


def test_double_inversion_changes_the_patch_nowhere():
    """warpAffine's coordinates from the matrix inverted twice against the same tables from the matrix itself"""
    img = image(4, 60, 80, 3)
    m = R.similarity(23.0, 0.83, 11.3, 7.9)
    p, _ = R.warp_affine(img, m, 50, 40)
    orig = R.warp_matrix
    R.warp_matrix = lambda mm: [float(v) for v in mm]
    try:
        q, _ = R.warp_affine(img, m, 50, 40)
    finally:
        R.warp_matrix = orig
    assert np.abs(np.array(orig(m)) - m).max() < 1e-12 and (p == q).all()
