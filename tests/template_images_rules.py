"""The model of TemplateMatcher::match from the decoded images to the score (src/templatematcher.cpp:105-374), composed
from what the repository already trusts, and the fixtures the CPU and the GPU tests of cbird_amd/csrc/tmimages.hip share.

  candScale / sizes   the float32 arithmetic of :182-192 and sizeScaleFactor (src/cvutil.cpp:1952-1953), in numpy
  resize              Oracle.resize_lanczos4 on each channel plane
  grey                PrestageOracle.bgr2gray
  ORB                 OrbOracle.detect + compute (the synthetic pattern, libstdc++'s retain order: set on both sides)
  match               brute-force popcount, inside a query ascending (distance, train row)
  gather              numpy, from the keypoints as compute() leaves them
  estimates .. score  template_match_rules.template_match with PrestageOracle.template_score
Nothing here is a new tolerance: everything is compared bit for bit but the matrices (template_match_rules.m_tolerance)."""
import numpy as np

import template_match_rules as R

F32 = np.float32
(SCORED, NO_TEMPLATE_KEYPOINTS, NO_KEYPOINTS, NO_MATCHES, FEW_POINTS, NO_TRANSFORM, EMPTY_RESIZE) = range(7)
DEFAULTS = dict(needle=100, haystack=1000, cv_thresh=25, scale_pct=200)  # src/index.h:76-84
_cache = {}


# ---- :182-192, cvutil.cpp:1952-1953 --------------------------------------------------------------------------------------
def max_size(t_size, pct):
    """int maxSize = tSize * params.tmScalePct / 100.0: a double product and quotient, truncated"""
    return int(float(t_size * pct) / 100.0)


def cand_target(tw, th, w, h, pct):
    """-> (candScale float32, target w, target h, resized)"""
    scale, dw, dh, resized = F32(1.0), w, h, False
    if th * tw < h * w:
        c_size, t_size = max(w, h), max(th, tw)
        ms = max_size(t_size, pct)
        if c_size > ms:
            scale = F32(ms) / F32(c_size)
            dw, dh, resized = int(F32(w) * scale), int(F32(h) * scale), True
    assert isinstance(scale, F32)
    return scale, dw, dh, resized


# ---- the stages ----------------------------------------------------------------------------------------------------------
def oracles():
    if "orc" not in _cache:
        import oracle
        from cbird_amd.orb import synthetic_pattern

        o = oracle.OrbOracle()
        o.set_pattern(synthetic_pattern())
        o.set_retain_order(1)
        _cache["orc"] = (oracle.Oracle(), oracle.PrestageOracle(), o)
    return _cache["orc"]


def resize(img, dw, dh):
    orc = oracles()[0]
    if img.ndim == 2:
        return orc.resize_lanczos4(img, dw, dh)
    return np.stack([orc.resize_lanczos4(np.ascontiguousarray(img[..., c]), dw, dh) for c in range(img.shape[2])], -1)


def gray(img):
    return img if img.ndim == 2 else oracles()[1].bgr2gray(img)


def orb(img, nfeatures):
    """-> (x, y float32 [k, 2] as compute() leaves them, descriptors uint8 [k, 32])"""
    o = oracles()[2]
    g = np.ascontiguousarray(gray(img))
    kp, desc = o.compute(g, o.detect(g, nfeatures))
    return np.stack([kp["x"], kp["y"]], 1).astype(F32).reshape(-1, 2), desc.reshape(-1, 32)


_POP = np.array([bin(v).count("1") for v in range(256)], np.int32)


def radius_match(train, queries, max_dist):
    """-> int32 [k, 3] (query row, train row, distance): every pair with distance <= max_dist, by query row, inside a
    query ascending (distance, train row)"""
    out = []
    train = np.asarray(train, np.uint8).reshape(-1, 32)
    for q, row in enumerate(np.asarray(queries, np.uint8).reshape(-1, 32)):
        if not len(train):
            break
        d = _POP[train ^ row].sum(1)
        hit = np.flatnonzero(d <= max_dist)
        hit = hit[np.argsort(d[hit], kind="stable")]
        out.append(np.stack([np.full(len(hit), q), hit, d[hit]], 1).astype(np.int32))
    return np.concatenate(out).reshape(-1, 3) if out else np.zeros((0, 3), np.int32)


def gather(records, tmpl_xy, cand_xy):
    return tmpl_xy[records[:, 1]].reshape(-1, 2), cand_xy[records[:, 0]].reshape(-1, 2)


# ---- the chain -----------------------------------------------------------------------------------------------------------
def template_match_images(tmpl, cands, needle=100, haystack=1000, cv_thresh=25, scale_pct=200):
    """one dict per candidate: status, scale, w, h, n_keypoints, n_matches, records, tmpl_pts, match_pts, work (the image
    after the resize) and r (template_match_rules.template_match's dict; None where the chain never got that far)"""
    th, tw = tmpl.shape[:2]
    score = oracles()[1].template_score
    t_xy, t_desc = orb(tmpl, needle)
    out = []
    for img in cands:
        h, w = img.shape[:2]
        if len(t_desc) == 0:
            out.append(dict(status=NO_TEMPLATE_KEYPOINTS, scale=F32(1), w=w, h=h, n_keypoints=0, n_matches=0, r=None))
            continue
        scale, dw, dh, resized = cand_target(tw, th, w, h, scale_pct)
        if dw <= 0 or dh <= 0:
            out.append(dict(status=EMPTY_RESIZE, scale=scale, w=dw, h=dh, n_keypoints=0, n_matches=0, r=None))
            continue
        work = resize(img, dw, dh) if resized else img
        c_xy, c_desc = orb(work, haystack)
        rec = radius_match(t_desc, c_desc, cv_thresh)
        a, b = gather(rec, t_xy, c_xy)
        r = R.template_match(tmpl, [work], a, [b], [scale], score)[0]
        status = (NO_KEYPOINTS if len(c_desc) == 0 else NO_MATCHES if len(rec) == 0 else FEW_POINTS if len(rec) < 3
                  else SCORED if r["found"] else NO_TRANSFORM)
        out.append(dict(status=status, scale=scale, w=dw, h=dh, n_keypoints=len(c_desc), n_matches=len(rec), records=rec,
                        tmpl_pts=a, match_pts=b, work=work, resized=resized, r=r))
    return out


# ---- the chain's fixture -------------------------------------------------------------------------------------------------
TW, TH = 160, 128
NAMES = ["copy", "shifted", "enlarged_2_5", "rotated_10_scaled_0_8", "unrelated", "flat", "inside_border", "shifted_noisy",
         "enlarged_2_2", "speck"]
CHAIN_SEED = {1: 2, 3: 1, 4: 1}  # per channel count: the first seeds at which test_template_images_rules' conditions hold


def _channels(img, ch):
    return img if ch != 1 or img.ndim == 2 else img[..., 0]


def chain_images(ch, seed=None):
    """(template 160 x 128, candidates in the order of NAMES)"""
    seed = CHAIN_SEED[ch] if seed is None else seed
    rng = np.random.default_rng(1000 * ch + seed)
    tmpl = R.scene(rng, TH, TW, ch)
    t3 = tmpl.reshape(TH, TW, ch)

    def paste(cw, chh, x0, y0, noise=0):
        canvas = np.full((chh, cw, ch), 90, np.int32)
        canvas[y0:y0 + TH, x0:x0 + TW] = t3
        if noise:
            canvas += rng.integers(-noise, noise + 1, canvas.shape)
        return np.clip(canvas, 1, 255).astype(np.uint8)

    def warped(deg, sc, tx, ty, cw, chh):
        return R.warp_affine(tmpl, R.invert(R.similarity(deg, sc, tx, ty)), cw, chh)[0].reshape(chh, cw, ch)

    speck = np.full((TH, TW, ch), 90, np.uint8)
    speck[40:52, 60:72] = t3[40:52, 60:72]
    cands = [t3.copy(), paste(200, 170, 23, 17), warped(0, 2.5, 10.0, 10.0, 420, 340), warped(10, 0.8, 40.0, 12.0, 200, 170),
             R.scene(np.random.default_rng(77 + seed), 150, 180, ch).reshape(150, 180, ch),
             np.full((TH, TW, ch), 100, np.uint8), t3[30:70, 50:90].copy(), paste(200, 170, 9, 30, noise=2),
             warped(0, 2.2, 4.0, 6.0, 360, 300), speck]
    assert len(cands) == len(NAMES)
    return tmpl, [np.ascontiguousarray(_channels(c, ch)) if ch == 1 else np.ascontiguousarray(c) for c in cands]


def chain_fixture(ch):
    """(template, candidates, the model's results), built once per channel count and never written to"""
    if ("chain", ch) not in _cache:
        tmpl, cands = chain_images(ch)
        _cache[("chain", ch)] = (tmpl, cands, template_match_images(tmpl, cands))
    return _cache[("chain", ch)]


def chain_conditions(model):
    """what keeps the GPU comparison from passing on an all-empty fixture; -> the list of conditions that do NOT hold"""
    st = [m["status"] for m in model]
    bad = []
    if sum(s == SCORED for s in st) < 3:
        bad.append("fewer than 3 scored")
    if not any(m["status"] == SCORED and m["resized"] for m in model):
        bad.append("no scored candidate was resized")
    if NO_KEYPOINTS not in st:
        bad.append("no candidate without keypoints")
    if not {NO_MATCHES, FEW_POINTS, NO_TRANSFORM} & set(st):
        bad.append("no candidate without a match")
    if not (model[0]["status"] == SCORED and model[0]["r"]["score"] == 0):
        bad.append("the exact copy does not score 0")
    return bad


# ---- the match stage's synthetic descriptors -----------------------------------------------------------------------------
QUERY_COUNTS = [0, 1, 64, 65, 1000]  # candidates of one call; then four more with exactly 0, 1, 2 and 3 matches
KP_CAP = 1000


def flip(row, bits, rng):
    """a copy of the 32-byte row with exactly `bits` bits flipped"""
    out = row.copy()
    for b in rng.choice(256, bits, replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def match_case(n_train, max_dist, seed=1):
    """(train [n_train, 32], train_xy, desc [n, KP_CAP, 32], xy [n, KP_CAP, 2], counts [n]): random rows are ~128 bits
    apart, so the only pairs within a max_dist below 256 are the planted ones: queries at exactly max_dist (in) and
    max_dist + 1 (out) of a train row, and copies of DUPLICATED train rows (equal distances: the order is by train row)."""
    rng = np.random.default_rng(seed * 7919 + n_train * 31 + max_dist)
    train = rng.integers(0, 256, (n_train, 32), dtype=np.uint8)
    if n_train >= 3:
        train[n_train - 1] = train[0]  # duplicates, far apart and adjacent
        train[2] = train[1]
    counts = QUERY_COUNTS + [5, 5, 5, 5]
    n = len(counts)
    desc = rng.integers(0, 256, (n, KP_CAP, 32), dtype=np.uint8)
    xy = rng.uniform(0, 400, (n, KP_CAP, 2)).astype(F32)
    train_xy = rng.uniform(0, 400, (n_train, 2)).astype(F32)
    far = min(max_dist + 1, 256)
    for i, c in enumerate(QUERY_COUNTS):  # planted neighbours in the ragged candidates
        for j in range(0, c, 7):
            t = int(rng.integers(0, n_train))
            desc[i, j] = flip(train[t], max_dist if (j // 7) % 2 == 0 else far, rng)
    for k in range(4):  # exactly k matches in total (when max_dist < 100: random rows stay out)
        i = len(QUERY_COUNTS) + k
        for j in range(k):
            desc[i, j] = flip(train[n_train // 2], max_dist, rng)
        # (a train row that is a duplicate would give two pairs per query: n_train // 2 is one only for n_train 3..5)
    return train, train_xy, desc, xy, np.array(counts, np.uint32)


def match_model(train, train_xy, desc, xy, counts, max_dist):
    """-> (first uint64 [n + 1], records int32 [total, 3], tmpl_pts, match_pts)"""
    recs, first = [], [0]
    a, b = [], []
    for i, c in enumerate(counts):
        r = radius_match(train, desc[i, :c], max_dist)
        ta, tb = gather(r, train_xy, xy[i])
        recs.append(r), a.append(ta), b.append(tb)
        first.append(first[-1] + len(r))
    return (np.array(first, np.uint64), np.concatenate(recs), np.concatenate(a).astype(F32), np.concatenate(b).astype(F32))
