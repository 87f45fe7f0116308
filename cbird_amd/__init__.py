"""cbird_amd -- MI355X-native perceptual-hash build + Hamming nearest-neighbour find for cbird.

Only the hot path: HIP kernels + C-ABI in ``csrc/`` / ``include/cbird_hip.h`` and
this thin host mirror of the reference's Index plugin surface.  Importing the package does not
load the shared library; the first call does, and fails loudly when it (or a gfx950 device) is
missing.
"""
from ._lib import CbhError, lib, require_device  # noqa: F401
from .alignment import align_spatial, align_temporal, alignment_transform  # noqa: F401
from .database import clusters, merge, multi_search, sort_similar, sort_similar_batch, video_coverage, video_segments  # noqa: F401
from .demosaic import demosaic, edge_maps, grid_lines, grid_tiles  # noqa: F401
from .difference import auto_contrast, difference_images  # noqa: F401
from .hashing import dct_hash64, dct_hash64_batch, estimate_rigid, template_match, warp_affine  # noqa: F401
from .index import DctFeaturesIndex, DctHashIndex, Match, MatchRange, Media, SearchParams  # noqa: F401
from .quality import quality_planes, quality_scores  # noqa: F401

__all__ = ["CbhError", "lib", "require_device", "dct_hash64", "dct_hash64_batch", "DctHashIndex",
           "DctFeaturesIndex", "quality_scores", "quality_planes", "estimate_rigid", "warp_affine", "template_match",
           "auto_contrast", "difference_images", "align_spatial", "align_temporal", "alignment_transform",
           "demosaic", "edge_maps", "grid_lines", "grid_tiles", "sort_similar", "sort_similar_batch", "clusters",
           "merge", "multi_search", "video_coverage", "video_segments",
           "Match", "MatchRange", "Media", "SearchParams"]
