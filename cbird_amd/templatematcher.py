"""TemplateMatcher (src/templatematcher.{h,cpp}): the post-filter behind -p.tm 1.  match() restates the front of
TemplateMatcher::match -- the md5-pair cache (:50-103), the threshold and the sort (:378-435) -- around ONE
hashing.template_match_images call for all the candidates the cache does not answer.  match_groups() is match() for a
list of (template, group) at once -- what Database::similar does once per needle (src/database.cpp:1418) -- around ONE
hashing.template_match_pairs call for every pair of every group.

A media here is any object with ``md5`` (str, may be empty), ``score`` (written) and ``image`` (a uint8 array, or a
callable that returns one or None: Media::loadImage); ``roi`` and ``transform`` are written when the object has them."""
from __future__ import annotations

import threading

import numpy as np

INT_MAX = (1 << 31) - 1


def _device_scorer(tmpl, cands, params):
    from .hashing import template_match_images

    return template_match_images(tmpl, cands, params)


def _device_pair_scorer(images, pair_tmpl, pair_cand, params):
    from .hashing import template_match_pairs

    return template_match_pairs(images, pair_tmpl, pair_cand, params)


def _pairs_through(scorer):
    """a pair scorer from a per-template scorer: one scorer call per distinct template, in first-appearance order"""

    def pair_scorer(images, pair_tmpl, pair_cand, params):
        from .hashing import TEMPLATE_IMAGE_RESULT_DTYPE

        out = np.zeros(len(pair_tmpl), TEMPLATE_IMAGE_RESULT_DTYPE)
        by_tmpl: dict = {}
        for p, t in enumerate(pair_tmpl):
            by_tmpl.setdefault(int(t), []).append(p)
        for t, ps in by_tmpl.items():
            res = scorer(images[t], [images[int(pair_cand[p])] for p in ps], params)
            for p, r in zip(ps, res):
                out[p] = r
        return out

    return pair_scorer


def _image(m):
    img = m.image() if callable(m.image) else m.image
    return None if img is None or np.asarray(img).size == 0 else np.asarray(img)


class TemplateMatcher:
    def __init__(self, scorer=None, pair_scorer=None) -> None:
        """scorer(tmpl, cands, params) -> TEMPLATE_IMAGE_RESULT_DTYPE [len(cands)]; the default runs on the device.
        pair_scorer(images, pair_tmpl, pair_cand, params) -> TEMPLATE_IMAGE_RESULT_DTYPE [len(pair_tmpl)], what
        match_groups calls once; the default is the device's hashing.template_match_pairs, or, where only `scorer` is
        given, that scorer once per distinct template."""
        self._scorer = scorer or _device_scorer
        self._pair_scorer = pair_scorer or (_pairs_through(scorer) if scorer else _device_pair_scorer)
        self._cache: dict[str, int] = {}
        self._lock = threading.Lock()  # (the reference's QReadWriteLock)

    def match(self, tmpl, group, params):
        """TemplateMatcher::match(tmplMedia, group, params): returns the members of `group` that score below
        params.tmThresh, their score set, sorted by score (the reference rewrites `group` in place)."""
        return self._match(tmpl, group, params, _image,
                           lambda timg, loaded: self._scorer(timg, [img for _, img in loaded], params))

    def _not_cached(self, tmpl, group, good, params):
        """:51-91: (use_cache, the members the cache does not answer); the answered ones get their score, and go to
        `good` (where it is a list) when it is below the threshold"""
        use_cache = bool(tmpl.md5) and all(bool(m.md5) for m in group)  # :51-62
        not_cached = []
        if use_cache:  # :66-91: one key per pair of images, either order
            with self._lock:
                for m in group:
                    for key in (m.md5 + tmpl.md5, tmpl.md5 + m.md5):
                        if key in self._cache:
                            if good is not None:
                                m.score = self._cache[key]
                                if m.score < params.tmThresh:
                                    good.append(m)
                            break
                    else:
                        not_cached.append(m)
        else:
            not_cached = list(group)
        return use_cache, not_cached

    def _match(self, tmpl, group, params, image, score):
        """match() with the image loader and score(template image, [(media, image)]) -> results given"""
        from .hashing import TM_FEW_POINTS, TM_NO_MATCHES, TM_NO_TRANSFORM, TM_SCORED

        group = list(group)
        if not group:
            return []
        good = []
        use_cache, not_cached = self._not_cached(tmpl, group, good, params)
        if not not_cached:  # :98-103
            return sorted(good, key=lambda m: m.score)
        timg = image(tmpl)
        if timg is None:  # :107-111 "failure to load tmpl image": the group comes back empty
            return []
        loaded = [(m, image(m)) for m in not_cached]
        loaded = [(m, img) for m, img in loaded if img is not None]  # :166-170: skipped, nothing cached
        if loaded:
            res = score(timg, loaded)
            for (m, _), r in zip(loaded, res):
                status = int(r["status"])
                if status not in (TM_SCORED, TM_NO_MATCHES, TM_FEW_POINTS, TM_NO_TRANSFORM):
                    continue  # :210-213 continues without caching; :127-130 returns; an empty resize throws
                key = m.md5 + tmpl.md5 if use_cache else "invalid-cache-key"  # :163-164
                dist = int(r["r"]["score"]) if status == TM_SCORED else INT_MAX  # :233, :258, :271
                if status == TM_SCORED:  # :378-381
                    m.score = dist
                    if hasattr(m, "roi"):
                        m.roi = np.array(r["r"]["roi"]).reshape(4, 2)
                    if hasattr(m, "transform") and r["r"]["tx_found"]:
                        m.transform = np.array(r["r"]["tx"]).reshape(2, 3)
                    if dist < params.tmThresh:
                        good.append(m)
                with self._lock:
                    self._cache[key] = dist
        return sorted(good, key=lambda m: m.score)  # :434-435 (Python's sort is stable where std::sort need not be)

    def match_groups(self, tmpls, groups, params):
        """[self.match(t, g, params) for t, g in zip(tmpls, groups)] -- the same lists, the same roi / transform writes and
        the same cache afterwards -- with ONE pair scorer call (none when the cache answers everything).  The groups are
        taken in the order given (the reference fills its cache from a thread pool: which of (A, B) and (B, A) it computes
        is a race there).  Every ordered (template, candidate) pair the cache does not answer AS IT STANDS ON ENTRY is sent,
        once; match()'s logic is then replayed group by group on the host with the scores looked up.  A pair whose key an
        earlier group has cached by then takes the cached score; a pair whose earlier twin ended in a status that is not
        cached (:210-213, a template without keypoints, an empty resize) uses its own result.  An image is loaded once."""
        tmpls, groups = list(tmpls), [list(g) for g in groups]
        if len(tmpls) != len(groups):
            raise ValueError("one template per group")
        images: dict = {}  # id(media) -> its image or None (the objects stay alive in tmpls / groups)

        def image(m):
            if id(m) not in images:
                images[id(m)] = _image(m)
            return images[id(m)]

        def ident(m):  # what makes two media the same image: the md5 where there is one
            return ("md5", m.md5) if m.md5 else ("id", id(m))

        table, rows, pt, pc, sent = [], {}, [], [], {}

        def row(m):
            if ident(m) not in rows:
                rows[ident(m)] = len(table)
                table.append(image(m))
            return rows[ident(m)]

        for t, g in zip(tmpls, groups):
            if not g:
                continue
            _, not_cached = self._not_cached(t, g, None, params)
            if not not_cached or image(t) is None:
                continue
            for m in not_cached:
                if image(m) is not None and (ident(t), ident(m)) not in sent:
                    sent[(ident(t), ident(m))] = len(pt)
                    pt.append(row(t)), pc.append(row(m))
        res = self._pair_scorer(table, np.array(pt, np.uint32), np.array(pc, np.uint32), params) if pt else None
        return [self._match(t, g, params, image,
                            lambda timg, loaded, t=t: [res[sent[(ident(t), ident(m))]] for m, _ in loaded])
                for t, g in zip(tmpls, groups)]
