"""TemplateMatcher (src/templatematcher.{h,cpp}): the post-filter behind -p.tm 1.  match() restates the front of
TemplateMatcher::match -- the md5-pair cache (:50-103), the threshold and the sort (:378-435) -- around ONE
hashing.template_match_images call for all the candidates the cache does not answer.

A media here is any object with ``md5`` (str, may be empty), ``score`` (written) and ``image`` (a uint8 array, or a
callable that returns one or None: Media::loadImage); ``roi`` and ``transform`` are written when the object has them."""
from __future__ import annotations

import threading

import numpy as np

INT_MAX = (1 << 31) - 1


def _device_scorer(tmpl, cands, params):
    from .hashing import template_match_images

    return template_match_images(tmpl, cands, params)


def _image(m):
    img = m.image() if callable(m.image) else m.image
    return None if img is None or np.asarray(img).size == 0 else np.asarray(img)


class TemplateMatcher:
    def __init__(self, scorer=None) -> None:
        """scorer(tmpl, cands, params) -> TEMPLATE_IMAGE_RESULT_DTYPE [len(cands)]; the default runs on the device"""
        self._scorer = scorer or _device_scorer
        self._cache: dict[str, int] = {}
        self._lock = threading.Lock()  # (the reference's QReadWriteLock)

    def match(self, tmpl, group, params):
        """TemplateMatcher::match(tmplMedia, group, params): returns the members of `group` that score below
        params.tmThresh, their score set, sorted by score (the reference rewrites `group` in place)."""
        from .hashing import TM_FEW_POINTS, TM_NO_MATCHES, TM_NO_TRANSFORM, TM_SCORED

        group = list(group)
        if not group:
            return []
        use_cache = bool(tmpl.md5) and all(bool(m.md5) for m in group)  # :51-62
        good, not_cached = [], []
        if use_cache:  # :66-91: one key per pair of images, either order
            with self._lock:
                for m in group:
                    for key in (m.md5 + tmpl.md5, tmpl.md5 + m.md5):
                        if key in self._cache:
                            m.score = self._cache[key]
                            if m.score < params.tmThresh:
                                good.append(m)
                            break
                    else:
                        not_cached.append(m)
        else:
            not_cached = group
        if not not_cached:  # :98-103
            return sorted(good, key=lambda m: m.score)
        timg = _image(tmpl)
        if timg is None:  # :107-111 "failure to load tmpl image": the group comes back empty
            return []
        loaded = [(m, _image(m)) for m in not_cached]
        loaded = [(m, img) for m, img in loaded if img is not None]  # :166-170: skipped, nothing cached
        if loaded:
            res = self._scorer(timg, [img for _, img in loaded], params)
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
