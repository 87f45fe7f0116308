"""The model and the fixture of the grouped template match (cbh_template_match_pairs, cbird_amd/csrc/tmimages.hip): pair p of
one image table is template_images_rules' chain for template images[pair_tmpl[p]] and the one candidate
images[pair_cand[p]].  Nothing new is modelled here: the chain's model treats every candidate on its own, so the pairs of
one template are handed to it together.

No template below 64 x 64 is in the fixture: the model finds no keypoint on crops of the template of 40 x 40, 62 x 50 and
63 x 63 (ORB's edge threshold leaves no room), so such a template would only be a second flat one."""
import numpy as np

import template_images_rules as M

_cache = {}

# the table: the chain fixture's template and candidates, a crop of the template with an odd width, and the strip whose
# resize target has a side of 0
TMPL, COPY, SHIFTED, ENLARGED, ROTATED, UNRELATED, FLAT, BORDER, NOISY, ENLARGED_2_2, SPECK, CROP, THIN = range(13)
CROP_W, CROP_H, CROP_X, CROP_Y = 131, 97, 20, 15
# (template, candidate): the pairs of TMPL, SHIFTED and FLAT are not adjacent; CROP has exactly one
PAIRS = [(TMPL, COPY), (TMPL, SHIFTED), (CROP, TMPL), (TMPL, ENLARGED), (SHIFTED, TMPL), (TMPL, ROTATED), (FLAT, COPY),
         (TMPL, UNRELATED), (TMPL, TMPL), (TMPL, FLAT), (SHIFTED, NOISY), (TMPL, BORDER), (FLAT, TMPL), (TMPL, NOISY),
         (TMPL, ENLARGED_2_2), (TMPL, THIN), (TMPL, SPECK), (FLAT, FLAT)]


def template_match_pairs(images, pair_tmpl, pair_cand, **kw):
    """-> one dict per pair: M.template_match_images(images[t], [images[c]], **kw)[0]"""
    out = [None] * len(pair_tmpl)
    by_tmpl = {}
    for p, t in enumerate(pair_tmpl):
        by_tmpl.setdefault(int(t), []).append(p)
    for t, ps in by_tmpl.items():
        for p, r in zip(ps, M.template_match_images(images[t], [images[int(pair_cand[p])] for p in ps], **kw)):
            out[p] = r
    return out


def pairs_images(ch):
    tmpl, cands = M.chain_images(ch)
    crop = np.ascontiguousarray(tmpl[CROP_Y:CROP_Y + CROP_H, CROP_X:CROP_X + CROP_W])
    thin = np.full((8, 3000) + ((ch,) if ch > 1 else ()), 77, np.uint8)
    return [tmpl] + list(cands) + [crop, thin]


def pairs_fixture(ch):
    """(images, pair_tmpl, pair_cand, the model's results), built once per channel count and never written to"""
    if ch not in _cache:
        images = pairs_images(ch)
        pt = np.array([p[0] for p in PAIRS], np.uint32)
        pc = np.array([p[1] for p in PAIRS], np.uint32)
        _cache[ch] = (images, pt, pc, template_match_pairs(images, pt, pc))
    return _cache[ch]


def pairs_conditions(images, pt, pc, model):
    """what keeps the GPU comparison from passing on an easy fixture; -> the list of conditions that do NOT hold"""
    bad = []
    st = [m["status"] for m in model]
    tmpls = sorted(set(int(t) for t in pt))
    of = {t: [p for p in range(len(pt)) if pt[p] == t] for t in tmpls}
    ch = 1 if images[0].ndim == 2 else images[0].shape[2]
    if len({images[t].shape[:2] for t in tmpls}) < 3:
        bad.append("fewer than three template sizes")
    if not any(images[t].shape[1] % 2 == 1 and (images[t].shape[0] * images[t].shape[1] * ch) % 16 for t in tmpls):
        bad.append("no template with an odd width and a size that is no multiple of 16 bytes")
    flat = [t for t in tmpls if all(st[p] == M.NO_TEMPLATE_KEYPOINTS for p in of[t])]
    if not any(len(of[t]) >= 2 for t in flat):
        bad.append("no flat template with two pairs")
    for t in tmpls:
        if t not in flat and not any(st[p] == M.SCORED for p in of[t]):
            bad.append(f"template {t} has no scored pair")
        if t not in flat and any(st[p] == M.NO_TEMPLATE_KEYPOINTS for p in of[t]):
            bad.append(f"template {t} is flat in some pairs only")
    if not any(m["status"] == M.SCORED and m["resized"] for m in model):
        bad.append("no scored pair was resized")
    if not set(int(t) for t in pt) & set(int(c) for c in pc):
        bad.append("no image is both a template and a candidate")
    have = set(zip(pt.tolist(), pc.tolist()))
    if not any(a != b and (b, a) in have for a, b in have):
        bad.append("no (A, B) with its (B, A)")
    if not any(pt[p] == pc[p] and st[p] == M.SCORED and model[p]["r"]["score"] == 0 for p in range(len(pt))):
        bad.append("no pair of an image with itself that scores 0")
    if M.EMPTY_RESIZE not in st:
        bad.append("no empty resize")
    if M.NO_KEYPOINTS not in st:
        bad.append("no candidate without keypoints")
    if not {M.NO_MATCHES, M.FEW_POINTS, M.NO_TRANSFORM} & set(st):
        bad.append("no candidate without a match")
    if not any(len(ps) == 1 for ps in of.values()):
        bad.append("no template with exactly one pair")
    if not any(ps[-1] - ps[0] + 1 != len(ps) for ps in of.values()):
        bad.append("every template's pairs are adjacent")
    return bad
