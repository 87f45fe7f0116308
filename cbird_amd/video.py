"""Host-side mirror of DctVideoIndex / VideoIndex (src/dctvideoindex.{h,cpp}, src/videoindex.{h,cpp}).

  VideoIndex       frames + hashes of one video and the .vdx v2 file format (save/load/isValid)
  make_video_index the frame de-dup of Media::makeVideoIndex over a sequence of frame hashes
  VideoIndexer     Media::makeVideoIndex for frames pushed in chunks: autocrop + dctHash64 on the device, the
                   near-frame filter's state kept between pushes (host arrays or device tensors)
  DctVideoIndex    add/remove/count/find (findFrame for image needles, findVideo for video needles)

Compute and format code live in libcbird_hip.so (include/cbird_hip.h); nothing here falls back to CPU.
"""
from __future__ import annotations

import ctypes as C
import os
import warnings
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import CbhError, cbh_vmatch, check
from .index import Match, MatchRange, SearchParams

CBIRD_VERSION = "0.8.1"


@dataclass
class VideoIndex:
    """src/videoindex.h:40-67"""
    frames: list = field(default_factory=list)
    hashes: list = field(default_factory=list)

    def isEmpty(self) -> bool:
        return len(self.frames) == 0 or len(self.hashes) == 0

    def to_bytes(self) -> bytes:
        L = _lib.lib()
        f = np.ascontiguousarray(self.frames, np.int32)
        h = np.ascontiguousarray(self.hashes, np.uint64)
        n = L.cbh_vdx_encode(f.ctypes.data, h.ctypes.data, len(f), CBIRD_VERSION.encode(), None, 0)
        if n == 0:
            raise ValueError("invalid video index (first frame must be 0, frames strictly increasing)")
        buf = np.zeros(n, np.uint8)
        L.cbh_vdx_encode(f.ctypes.data, h.ctypes.data, len(f), CBIRD_VERSION.encode(), buf.ctypes.data, n)
        return buf.tobytes()

    def save(self, path: str) -> None:
        with open(path, "wb") as fp:
            fp.write(self.to_bytes())

    @staticmethod
    def from_bytes(data: bytes) -> "VideoIndex":
        L = _lib.lib()
        buf = np.frombuffer(data, np.uint8)
        cap = max(1, len(buf))
        f = np.zeros(cap, np.int32)
        h = np.zeros(cap, np.uint64)
        n = L.cbh_vdx_decode(buf.ctypes.data, len(buf), f.ctypes.data, h.ctypes.data, cap)
        if n < 0:
            raise ValueError(f"invalid .vdx data ({n})")
        return VideoIndex(f[:n].tolist(), [int(x) for x in h[:n]])

    @staticmethod
    def load(path: str) -> "VideoIndex":
        with open(path, "rb") as fp:
            return VideoIndex.from_bytes(fp.read())

    @staticmethod
    def isValid(path: str) -> bool:
        """VideoIndex::isValid (src/videoindex.cpp:90-104) -> verify_v2: header fields + the "cbir" trailer"""
        try:
            with open(path, "rb") as fp:
                data = fp.read()
        except OSError:
            return False
        buf = np.frombuffer(data, np.uint8)
        return bool(_lib.lib().cbh_vdx_verify(buf.ctypes.data, len(buf))) if len(buf) else False


def make_video_index(frame_hashes, threshold: int = 8) -> VideoIndex:
    """Media::makeVideoIndex (src/media.cpp:925-1037) given the per-frame dct hashes: keeps the frames the
    reference would store (videoThreshold default 8, src/scanner.h)."""
    L = _lib.lib()
    h = np.ascontiguousarray(frame_hashes, np.uint64)
    keep = np.zeros(max(1, len(h)), np.uint8)
    L.cbh_video_dedup(h.ctypes.data, len(h), int(threshold), keep.ctypes.data)
    ix = np.nonzero(keep[: len(h)])[0]
    return VideoIndex(ix.tolist(), [int(x) for x in h[ix]])


class VideoIndexer:
    """Media::makeVideoIndex (src/media.cpp:925-1037) fed by a decoder that produces frames in chunks.

        ix = VideoIndexer(threshold=8)              # IndexParams::videoThreshold; autocrop(img, 20) as at :961
        for chunk in decoder:                        # (n, h, w) uint8 numpy array or cuda tensor
            ix.push(chunk)
        video_index = ix.finish()

    resume = a VideoIndex written earlier (:929-936): frame numbering continues behind its last frame."""

    def __init__(self, threshold: int = 8, autocrop_range: int = 20, device: int = 0,
                 resume: VideoIndex | None = None) -> None:
        self._L = _lib.lib()
        self._h = self._L.cbh_vindexer_create(int(device), int(threshold), int(autocrop_range))
        if not self._h:
            raise CbhError(_lib.CBH_E_NODEVICE, "cbh_vindexer_create")
        self._device = int(device)
        if resume is not None and not resume.isEmpty():
            f = np.ascontiguousarray(resume.frames, np.int32)
            h = np.ascontiguousarray(resume.hashes, np.uint64)
            check(self._L.cbh_vindexer_resume(self._h, f.ctypes.data, h.ctypes.data, len(f)), "vindexer_resume")

    def __del__(self) -> None:
        if getattr(self, "_h", None):
            self._L.cbh_vindexer_destroy(self._h)
            self._h = None

    def push(self, frames) -> None:
        """n grey frames in decode order: (n, h, w) or (h, w); rows and frames may be strided, pixels contiguous"""
        if hasattr(frames, "data_ptr"):  # torch tensor
            t = frames if frames.dim() == 3 else frames[None]
            if t.dtype.itemsize != 1 or t.dim() != 3 or (t.shape[2] > 1 and t.stride(2) != 1):
                raise ValueError("frames: expected (n, h, w) uint8 with contiguous rows")
            n, h, w = t.shape
            if n == 0:
                return
            if t.is_cuda:
                if t.device.index != self._device:
                    raise ValueError(f"frames live on {t.device}, the indexer on device {self._device}")
                import torch
                torch.cuda.current_stream(t.device).synchronize()  # the indexer runs on its own stream
                check(self._L.cbh_vindexer_push_dev(self._h, t.data_ptr(), n, w, h, t.stride(1), t.stride(0)),
                      "vindexer_push_dev")
                return
            frames = t.numpy()
        a = np.asarray(frames)
        if a.ndim == 2:
            a = a[None]
        if a.dtype != np.uint8 or a.ndim != 3:
            raise ValueError("frames: expected (n, h, w) uint8")
        if a.shape[0] == 0:
            return
        if a.shape[2] > 1 and a.strides[2] != 1 or a.strides[1] < a.shape[2] or a.strides[0] < 0:
            a = np.ascontiguousarray(a)
        n, h, w = a.shape
        check(self._L.cbh_vindexer_push(self._h, a.ctypes.data, n, w, h, a.strides[1], a.strides[0]), "vindexer_push")

    @property
    def frames_seen(self) -> int:
        """makeVideoIndex's frameNumber: the number the next frame gets"""
        return int(self._L.cbh_vindexer_frames_seen(self._h))

    def finish(self) -> VideoIndex:
        n = int(self._L.cbh_vindexer_finish(self._h, None, None, 0))
        f = np.zeros(max(1, n), np.int32)
        h = np.zeros(max(1, n), np.uint64)
        got = int(self._L.cbh_vindexer_finish(self._h, f.ctypes.data, h.ctypes.data, n))
        if got != n:
            raise CbhError(_lib.CBH_E_INVAL, f"cbh_vindexer_finish: {got} != {n}")
        return VideoIndex(f[:n].tolist(), [int(x) for x in h[:n]])


@dataclass
class VideoSearchParams(SearchParams):
    """video fields of SearchParams (src/index.h:103-107)"""
    skipFrames: int = 300
    minFramesMatched: int = 30
    minFramesNear: int = 60
    videoRadix: int = 10  # `-p.vradix`; only honoured by DctVideoIndex(radix_compat=True), else the search is exact


# ---- coverage maps (cbird_amd/csrc/vcoverage.hip; the rules are in include/cbird_hip.h) ------------------------------
VCOVER_DTYPE = np.dtype([("src_frames_total", "<i8"), ("src_frames_covered", "<i8"), ("gap_len", "<i8"),
                         ("gap_begin", "<i4"), ("n_src", "<i4"), ("n_dst", "<i4"), ("n_covered", "<i4"),
                         ("n_low_detail", "<i4"), ("near_percent", "<i4"), ("src_in", "<i4"), ("dst_in", "<i4"),
                         ("len", "<i4"), ("dst_min", "<i4"), ("dst_max", "<i4"), ("reserved", "<i4")])  # cbh_vcover
VCOVER_FRAME_DTYPE = np.dtype([("src_frame", "<i4"), ("dst_frame", "<i4"), ("distance", "<i4")])  # cbh_vcover_frame
VCOVER_FIELDS = tuple(n for n in VCOVER_DTYPE.names if n != "reserved")


@dataclass
class VideoCoverage:
    """Which frames of a source video a destination video contains: cbh_vcover, and with maps the nearest destination
    frame and its distance for every considered source frame (``frames`` / ``dst_frames`` / ``distances``, None without)"""
    thresh: int = 0
    src_frames_total: int = 0
    src_frames_covered: int = 0
    gap_len: int = 0
    gap_begin: int = 0
    n_src: int = 0
    n_dst: int = 0
    n_covered: int = 0
    n_low_detail: int = 0
    near_percent: int = 0
    src_in: int = -1
    dst_in: int = -1
    len: int = 0
    dst_min: int = -1
    dst_max: int = -1
    frames: np.ndarray | None = None
    dst_frames: np.ndarray | None = None
    distances: np.ndarray | None = None

    def contains(self, min_percent: float = 100) -> bool:
        """the destination holds at least min_percent of the source, counted in frames of the source's own numbering"""
        return self.src_frames_covered * 100 >= min_percent * self.src_frames_total

    def percent(self) -> int:
        return self.src_frames_covered * 100 // self.src_frames_total if self.src_frames_total else 0

    def spans(self) -> np.ndarray:
        """the span of every considered frame: up to the next one, and for the last what src_frames_total leaves"""
        if self.frames is None:
            raise ValueError("this VideoCoverage was made without maps")
        f = self.frames.astype(np.int64)
        if len(f) == 0:
            return f
        return np.append(np.diff(f), self.src_frames_total - (f[-1] - f[0]))

    def ranges(self, covered: bool = True) -> list:
        """the runs of consecutive considered frames that are covered (or are not) as (first_frame, length) in source
        frame numbers; the length is the sum of the run's spans"""
        spans = self.spans()
        flag = (self.distances < self.thresh) == bool(covered)
        out = []
        i, n = 0, len(flag)
        while i < n:
            if not flag[i]:
                i += 1
                continue
            j = i
            while j < n and flag[j]:
                j += 1
            out.append((int(self.frames[i]), int(spans[i:j].sum())))
            i = j
        return out


def _coverage_results(summaries, fmap, offs, thresh):
    out = []
    for k, s in enumerate(summaries):
        c = VideoCoverage(int(thresh), **{n: int(s[n]) for n in VCOVER_FIELDS})
        if fmap is not None:
            m = fmap[int(offs[k]):int(offs[k + 1])]
            c.frames, c.dst_frames, c.distances = m["src_frame"].copy(), m["dst_frame"].copy(), m["distance"].copy()
        out.append(c)
    return out


def _coverage_call(call, n_pairs, maps, what):
    """the capacity protocol of cbh_video_coverage: the sizes come back with CBH_E_OVERFLOW, the second call fills"""
    summaries = np.zeros(max(1, n_pairs), VCOVER_DTYPE)
    offs = np.zeros(n_pairs + 1, np.uint64)
    if not maps:
        check(call(summaries.ctypes.data, None, 0, offs.ctypes.data), what)
        return summaries[:n_pairs], None, offs
    fmap = np.zeros(1, VCOVER_FRAME_DTYPE)
    rc = call(summaries.ctypes.data, fmap.ctypes.data, 0, offs.ctypes.data)
    if rc == _lib.CBH_E_OVERFLOW:
        fmap = np.zeros(int(offs[-1]), VCOVER_FRAME_DTYPE)
        rc = call(summaries.ctypes.data, fmap.ctypes.data, len(fmap), offs.ctypes.data)
    check(rc, what)
    return summaries[:n_pairs], fmap, offs


def video_coverage(videos, pairs, thresh: int, skip_frames: int = 0, maps: bool = True, device: int = 0):
    """cbh_video_coverage for explicit lists: videos = [(frames, hashes), ...], pairs = [(source, destination), ...] as
    indexes into it.  One VideoCoverage per pair.  No index is involved: a needle outside the database works as well."""
    L = _lib.lib()
    videos = list(videos)
    f = np.concatenate([np.asarray(v[0], np.int32) for v in videos] or [np.zeros(0, np.int32)])
    h = np.concatenate([np.asarray(v[1], np.uint64) for v in videos] or [np.zeros(0, np.uint64)])
    o = np.zeros(len(videos) + 1, np.uint64)
    np.cumsum([len(v[0]) for v in videos], out=o[1:])
    p = np.ascontiguousarray(np.asarray(list(pairs), np.uint32).reshape(-1, 2))

    def call(s, m, cap, offs):
        return L.cbh_video_coverage(int(device), f.ctypes.data, h.ctypes.data, o.ctypes.data, len(videos), p.ctypes.data,
                                    len(p), int(thresh), int(skip_frames), s, m, cap, offs)

    return _coverage_results(*_coverage_call(call, len(p), maps, "video_coverage"), thresh)


# ---- offsets and segments (cbird_amd/csrc/vsegments.hip; the rules are in include/cbird_hip.h) ------------------------
VSEGMENT_DTYPE = np.dtype([("span_sum", "<i8"), ("offset", "<i4"), ("n_frames", "<i4"), ("src_first", "<i4"),
                           ("src_last", "<i4"), ("dst_first", "<i4"), ("dst_last", "<i4")])  # cbh_vsegment
VSEGMENTS_DTYPE = np.dtype([("src_frames_total", "<i8"), ("src_frames_aligned", "<i8"), ("n_src", "<i4"), ("n_dst", "<i4"),
                            ("n_segments", "<i4"), ("n_aligned", "<i4"), ("monotone", "<i4"), ("src_in", "<i4"),
                            ("dst_in", "<i4"), ("len", "<i4")])  # cbh_vsegments
VSEGMENT_FRAME_DTYPE = np.dtype([("src_frame", "<i4"), ("dst_frame", "<i4"), ("distance", "<i4"),
                                 ("segment", "<i4")])  # cbh_vsegment_frame
VSEGMENTS_MAX = 16  # CBH_VSEGMENTS_MAX


@dataclass
class VideoSegment:
    """One stretch of the source that lies in the destination at one frame-number offset (cbh_vsegment)"""
    span_sum: int = 0
    offset: int = 0
    n_frames: int = 0
    src_first: int = 0
    src_last: int = 0
    dst_first: int = 0
    dst_last: int = 0


@dataclass
class VideoSegments:
    """Where a source video lies in a destination video: cbh_vsegments, the segments in the order found (the best
    supported first), and with maps the chosen destination frame, its distance and the segment (-1, 65, -1 for a frame in
    none) of every considered source frame (``frames`` / ``dst_frames`` / ``distances`` / ``segment_of``, None without)"""
    src_frames_total: int = 0
    src_frames_aligned: int = 0
    n_src: int = 0
    n_dst: int = 0
    n_segments: int = 0
    n_aligned: int = 0
    monotone: int = 1
    src_in: int = -1
    dst_in: int = -1
    len: int = 0
    segments: list = field(default_factory=list)
    frames: np.ndarray | None = None
    dst_frames: np.ndarray | None = None
    distances: np.ndarray | None = None
    segment_of: np.ndarray | None = None

    def match_range(self):
        """segment 0's (src_in, dst_in, len) -- what seeks two players to the same picture; (-1, -1, 0) without one"""
        return self.src_in, self.dst_in, self.len

    def cut_list(self) -> list:
        """the segments in source order: where each stretch of the source starts, and by its offset where it went"""
        return sorted(self.segments, key=lambda g: g.src_first)

    def percent(self) -> int:
        """whole percent of the source's frames that lie in the destination at a consistent position"""
        return self.src_frames_aligned * 100 // self.src_frames_total if self.src_frames_total else 0


def _segments_results(summaries, segs, fmap, offs, max_segments):
    out = []
    for k, s in enumerate(summaries):
        r = VideoSegments(**{n: int(s[n]) for n in VSEGMENTS_DTYPE.names})
        r.segments = [VideoSegment(**{n: int(g[n]) for n in VSEGMENT_DTYPE.names})
                      for g in segs[k * max_segments:k * max_segments + r.n_segments]]
        if fmap is not None:
            m = fmap[int(offs[k]):int(offs[k + 1])]
            r.frames, r.dst_frames = m["src_frame"].copy(), m["dst_frame"].copy()
            r.distances, r.segment_of = m["distance"].copy(), m["segment"].copy()
        out.append(r)
    return out


def _segments_call(call, n_pairs, max_segments, maps, what):
    """the capacity protocol of cbh_video_coverage with one more array"""
    summaries = np.zeros(max(1, n_pairs), VSEGMENTS_DTYPE)
    segs = np.zeros(max(1, n_pairs * max_segments), VSEGMENT_DTYPE)
    offs = np.zeros(n_pairs + 1, np.uint64)
    if not maps:
        check(call(summaries.ctypes.data, segs.ctypes.data, None, 0, offs.ctypes.data), what)
        return summaries[:n_pairs], segs, None, offs
    fmap = np.zeros(1, VSEGMENT_FRAME_DTYPE)
    rc = call(summaries.ctypes.data, segs.ctypes.data, fmap.ctypes.data, 0, offs.ctypes.data)
    if rc == _lib.CBH_E_OVERFLOW:
        fmap = np.zeros(int(offs[-1]), VSEGMENT_FRAME_DTYPE)
        rc = call(summaries.ctypes.data, segs.ctypes.data, fmap.ctypes.data, len(fmap), offs.ctypes.data)
    check(rc, what)
    return summaries[:n_pairs], segs, fmap, offs


def video_segments(videos, pairs, thresh: int, skip_frames: int = 0, tol: int = 15, min_frames: int = 1,
                   max_segments: int = 4, maps: bool = True, device: int = 0):
    """cbh_video_segments for explicit lists: videos = [(frames, hashes), ...], pairs = [(source, destination), ...] as
    indexes into it.  One VideoSegments per pair."""
    L = _lib.lib()
    videos = list(videos)
    f = np.concatenate([np.asarray(v[0], np.int32) for v in videos] or [np.zeros(0, np.int32)])
    h = np.concatenate([np.asarray(v[1], np.uint64) for v in videos] or [np.zeros(0, np.uint64)])
    o = np.zeros(len(videos) + 1, np.uint64)
    np.cumsum([len(v[0]) for v in videos], out=o[1:])
    p = np.ascontiguousarray(np.asarray(list(pairs), np.uint32).reshape(-1, 2))

    def call(s, g, m, cap, offs):
        return L.cbh_video_segments(int(device), f.ctypes.data, h.ctypes.data, o.ctypes.data, len(videos), p.ctypes.data,
                                    len(p), int(thresh), int(skip_frames), int(tol), int(min_frames), int(max_segments),
                                    s, g, m, cap, offs)

    return _segments_results(*_segments_call(call, len(p), int(max_segments), maps, "video_segments"), int(max_segments))


class DctVideoIndex:
    """Detect similar videos with full-frame dct hashes (src/dctvideoindex.h:66-70)."""

    def __init__(self, device: int = 0, data_path: str | None = None, radix_compat: bool = False, shards=None,
                 _handle=None) -> None:
        # False: exact search (the reference's vradix = 0).  True: a needle frame only sees the entries of its
        # RadixMap bucket, (hash >> 1) & (2^videoRadix - 1) (src/tree/radix.h:135-141): the reference's
        # approximate candidate sets for `-p.vradix N`.
        self.radix_compat = bool(radix_compat)
        self._device = device
        self._L = _lib.lib()
        self._id = SearchParams.AlgoVideo
        self._data_path = data_path
        self._ids: set = set()  # the media ids the handle holds (what DctVideoIndex::_mediaId holds in the reference)
        self._loaded = False
        if _handle is not None:  # (slice(): the handle comes from cbh_vidx_slice)
            self._h = _handle
            return
        shards = shards if shards is not None else _lib.default_sharding()  # (device_mask, shards_per_device)
        self._h = self._L.cbh_vidx_create_sharded(shards[0], shards[1]) if shards else self._L.cbh_vidx_create(device)
        if not self._h:
            raise CbhError(_lib.CBH_E_NODEVICE, "cbh_vidx_create")

    def __del__(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.cbh_vidx_destroy(h)

    def id(self) -> int:
        return self._id

    def databaseId(self) -> int:
        return 0  # dctvideoindex.h:94

    def isLoaded(self) -> bool:
        return self._loaded

    def count(self) -> int:
        return int(self._L.cbh_vidx_count(self._h))

    def memoryUsage(self) -> int:
        """`_tree ? _tree->stats().memory : 0` (dctvideoindex.cpp:57-59): 0 until the first query builds the structure,
        then 8 + 6 bytes per entry"""
        return int(self._L.cbh_vidx_memory_usage(self._h))

    @property
    def handle(self):
        return self._h

    def _add_one(self, media_id: int, vi: VideoIndex) -> None:
        f = np.ascontiguousarray(vi.frames, np.int32)
        h = np.ascontiguousarray(vi.hashes, np.uint64)
        check(self._L.cbh_vidx_add_video(self._h, media_id, f.ctypes.data, h.ctypes.data, len(f)), "add_video")
        self._ids.add(int(media_id))

    def load(self, media_ids, data_path: str | None = None) -> None:
        """load(): `select id from media where type=video order by id` (:172-211); each id's frames come
        from <dataPath>/<id>.vdx (insertHashes :64-72); a missing file is warned about and skipped."""
        if data_path is not None:
            self._data_path = data_path
        for mid in media_ids:
            path = os.path.join(self._data_path, f"{mid}.vdx")
            if not os.path.exists(path):
                warnings.warn(f"index file missing: {path}")
                self._add_one(mid, VideoIndex())
            else:
                self._add_one(mid, VideoIndex.load(path))
        self._loaded = True

    def add(self, media) -> None:
        """add(): media carry (id, videoIndex) -- dctvideoindex.cpp:250-254"""
        for m in media:
            self._add_one(m.id, m.videoIndex)
        self._loaded = True

    def remove(self, ids) -> None:
        i = np.ascontiguousarray(list(ids), np.uint32)
        check(self._L.cbh_vidx_remove(self._h, i.ctypes.data, len(i)), "remove")
        self._ids.difference_update(int(x) for x in i)

    def slice(self, mediaIds) -> "DctVideoIndex":
        """DctVideoIndex::slice (dctvideoindex.cpp:389-397): "replicate what load() does, but use the subset" -- the
        videos the handle holds are copied from it (cbh_vidx_slice), only an id it does not hold is read from
        <dataPath>/<id>.vdx as load() does.

        Order: the videos the handle holds come first, in the order of mediaIds, and the ones it lacks follow, in the
        order of mediaIds too.  When every id is held (the usual case: load() adds an empty video even for a missing
        file) that is the order of mediaIds, as before; when some are not, the video indexes of the slice, and with
        them the order of equal-scored matches, can differ from a slice that read every file in the order of mediaIds.

        A data path is required even when every id is held, as it was when every id was read from its file."""
        if self._data_path is None:
            raise ValueError("slice() reads the .vdx files of media the index does not hold: the index needs a data path")
        ids = [int(x) for x in mediaIds]
        held = np.ascontiguousarray([i for i in ids if i in self._ids], np.uint32)
        h = self._L.cbh_vidx_slice(self._h, held.ctypes.data, len(held))
        if not h:
            raise CbhError(self._L.cbh_last_error_code() or _lib.CBH_E_HIP, "slice")
        copy = DctVideoIndex(self._device, self._data_path, self.radix_compat, _handle=h)
        copy._ids = set(int(x) for x in held)
        copy.load([i for i in ids if i not in self._ids])
        return copy

    @staticmethod
    def _matches(buf, n):
        return [Match(buf[i].id, buf[i].score, MatchRange(buf[i].src_in, buf[i].dst_in, buf[i].len))
                for i in range(n)]

    def _apply_radix(self, p) -> None:
        r = int(getattr(p, "videoRadix", 0)) if self.radix_compat else 0
        check(self._L.cbh_vidx_set_radix(self._h, r), "set_radix")

    def findFrame(self, needle, p: VideoSearchParams):
        self._apply_radix(p)
        hash_ = int(needle.dctHash)
        if hash_ == 0:
            warnings.warn(f"needle has no dct hash {needle.id} {needle.path}")
            return []
        cap = max(1, self.count())
        buf = (cbh_vmatch * cap)()
        n = C.c_size_t(0)
        src_in = getattr(needle, "matchRange", MatchRange()).dstIn
        check(self._L.cbh_vidx_find_frame(self._h, hash_, int(p.dctThresh), int(p.skipFrames), int(src_in), buf,
                                          cap, C.byref(n)), "find_frame")
        return self._matches(buf, n.value)

    def findVideo(self, needle, p: VideoSearchParams):
        self._apply_radix(p)
        vi = needle.videoIndex
        if vi is None or vi.isEmpty():
            warnings.warn(f"needle video index is empty: {needle.path}")
            return []
        f = np.ascontiguousarray(vi.frames, np.int32)
        h = np.ascontiguousarray(vi.hashes, np.uint64)
        cap = max(1, self.count())
        buf = (cbh_vmatch * cap)()
        n = C.c_size_t(0)
        check(self._L.cbh_vidx_find_video(self._h, f.ctypes.data, h.ctypes.data, len(f), needle.id,
                                          int(p.dctThresh), int(p.skipFrames), int(p.minFramesMatched),
                                          int(p.minFramesNear), int(bool(p.filterSelf)), buf, cap, C.byref(n)),
              "find_video")
        return self._matches(buf, n.value)

    def find(self, needle, p: VideoSearchParams):
        """dctvideoindex.cpp:277-289: image needle -> findFrame, video needle -> findVideo"""
        if getattr(needle, "videoIndex", None) is not None:
            return self.findVideo(needle, p)
        return self.findFrame(needle, p)

    def find_videos_batch(self, needles, p: VideoSearchParams):
        self._apply_radix(p)
        needles = list(needles)
        f = np.concatenate([np.asarray(m.videoIndex.frames, np.int32) for m in needles] or [np.zeros(0, np.int32)])
        h = np.concatenate([np.asarray(m.videoIndex.hashes, np.uint64) for m in needles] or [np.zeros(0, np.uint64)])
        o = np.zeros(len(needles) + 1, np.uint64)
        np.cumsum([len(m.videoIndex.frames) for m in needles], out=o[1:])
        i = np.ascontiguousarray([m.id for m in needles], np.uint32)
        out_offs = np.zeros(len(needles) + 1, np.uint64)
        cap = max(64, 8 * len(needles))
        while True:  # the library reports the full size in out_offs[-1] when cap was too small
            buf = (cbh_vmatch * cap)()
            rc = self._L.cbh_vidx_find_videos_batch(self._h, f.ctypes.data, h.ctypes.data, o.ctypes.data,
                                                    i.ctypes.data, len(needles), int(p.dctThresh),
                                                    int(p.skipFrames), int(p.minFramesMatched),
                                                    int(p.minFramesNear), int(bool(p.filterSelf)), buf, cap,
                                                    out_offs.ctypes.data)
            if rc == _lib.CBH_E_OVERFLOW and int(out_offs[-1]) > cap:
                cap = int(out_offs[-1])
                continue
            check(rc, "find_videos_batch")
            break
        return [self._matches(buf[int(out_offs[k]):int(out_offs[k + 1])], int(out_offs[k + 1] - out_offs[k]))
                for k in range(len(needles))]

    def find_frames_batch(self, needles, p: VideoSearchParams):
        """[findFrame(m, p) for m in needles] with one scan and one reduction on the device (cbh_vidx_find_frames_batch);
        a needle without a dct hash gets an empty list, as findFrame gives it"""
        self._apply_radix(p)
        needles = list(needles)
        for m in needles:
            if int(m.dctHash) == 0:
                warnings.warn(f"needle has no dct hash {m.id} {m.path}")
        h = np.ascontiguousarray([int(m.dctHash) for m in needles], np.uint64)
        s = np.ascontiguousarray([int(getattr(m, "matchRange", MatchRange()).dstIn) for m in needles], np.int32)
        out_offs = np.zeros(len(needles) + 1, np.uint64)
        cap = max(64, 8 * len(needles))
        while True:  # the library reports the full size in out_offs[-1] when cap was too small
            buf = (cbh_vmatch * cap)()
            rc = self._L.cbh_vidx_find_frames_batch(self._h, h.ctypes.data, s.ctypes.data, len(needles), int(p.dctThresh),
                                                    int(p.skipFrames), buf, cap, out_offs.ctypes.data)
            if rc == _lib.CBH_E_OVERFLOW and int(out_offs[-1]) > cap:
                cap = int(out_offs[-1])
                continue
            check(rc, "find_frames_batch")
            break
        return [self._matches(buf[int(out_offs[k]):int(out_offs[k + 1])], int(out_offs[k + 1] - out_offs[k]))
                for k in range(len(needles))]

    def coverage(self, pairs, p: VideoSearchParams, maps: bool = True):
        """Which frames of one video another contains (cbh_vidx_coverage): pairs = [(source media id, destination media
        id), ...] of videos the index holds, one VideoCoverage per pair, from one call -- every distinct video uploaded
        once.  p.dctThresh and p.skipFrames as in findVideo; the map is exact, videoRadix does not apply.  maps=False
        fetches the summaries only."""
        pairs = [(int(a), int(b)) for a, b in pairs]
        s = np.ascontiguousarray([a for a, _ in pairs], np.uint32)
        d = np.ascontiguousarray([b for _, b in pairs], np.uint32)

        def call(sums, m, cap, offs):
            return self._L.cbh_vidx_coverage(self._h, s.ctypes.data, d.ctypes.data, len(pairs), int(p.dctThresh),
                                             int(p.skipFrames), sums, m, cap, offs)

        return _coverage_results(*_coverage_call(call, len(pairs), maps, "vidx_coverage"), int(p.dctThresh))

    def segments(self, pairs, p: VideoSearchParams, tol: int = 15, min_frames: int | None = None, max_segments: int = 4,
                 maps: bool = True):
        """At which frame-number offsets one video lies in another (cbh_vidx_segments): pairs as in coverage(), one
        VideoSegments per pair, from one call.  p.dctThresh and p.skipFrames as in findVideo; tol is the slack in frames
        (findVideo's frameMargin), min_frames=None means p.minFramesMatched."""
        pairs = [(int(a), int(b)) for a, b in pairs]
        s = np.ascontiguousarray([a for a, _ in pairs], np.uint32)
        d = np.ascontiguousarray([b for _, b in pairs], np.uint32)
        least = int(p.minFramesMatched if min_frames is None else min_frames)

        def call(sums, g, m, cap, offs):
            return self._L.cbh_vidx_segments(self._h, s.ctypes.data, d.ctypes.data, len(pairs), int(p.dctThresh),
                                             int(p.skipFrames), int(tol), least, int(max_segments), sums, g, m, cap, offs)

        return _segments_results(*_segments_call(call, len(pairs), int(max_segments), maps, "vidx_segments"),
                                 int(max_segments))

    def entries(self, skip_frames: int) -> int:
        return int(self._L.cbh_vidx_entries(self._h, int(skip_frames)))
