"""MI355X-native language-Gaussian rasterizer (hot path of rpng/online_lang_splatting).

`from online_lang_splatting_amd import GaussianRasterizationSettings, GaussianRasterizer,
LanguageGaussianRasterizer` — or, as a drop-in, `import diff_gaussian_rasterization` (the
top-level shim package re-exports the same names).

Importing this package loads no native code; the first rasterizer call loads libolsr.so and
raises if it is missing (there is no CPU fallback).
"""
from ._abi import BINNING_ELLIPSE, BINNING_RECT, BWD_EXACT, BWD_REFERENCE  # noqa: F401
from .rasterizer import (GaussianRasterizationSettings, GaussianRasterizer,  # noqa: F401
                         LanguageGaussianRasterizer, rasterize_gaussians, rasterize_language_gaussians)

from .renderer import render  # noqa: F401,E402  (the caller-side façade: gaussian_renderer.render)
from .lang_query import LanguageDecoder, LanguageQuery  # noqa: F401,E402  (text queries on a rendered language map)
from .lang_encoder import LanguageEncoder  # noqa: F401,E402  (the general encoder 768 -> 32 ahead of the online autoencoder)
from .lang_single_stage import (SingleStageDecoder, SingleStageEncoder,  # noqa: F401,E402  (single_stage_ae: True: one
                                SingleStageQuery, SingleStageTargets)     # autoencoder 768 -> 15 -> 768, nothing online)
from .hr_net import HighResLanguageNet  # noqa: F401,E402  (the high-resolution feature net ahead of that encoder)
from .clip_trunk import ClipTrunk  # noqa: F401,E402  (the CLIP ConvNeXt image tower ahead of the HR net: a frame in, its maps out)
from .tsdf import TSDFVolume  # noqa: F401,E402  (TSDF fusion of depth and language maps into a 3-D map)
from .cloud_metrics import (chamfer_distance, chamfer_segments, earth_mover_distance,  # noqa: F401,E402  (the 3-D evaluation's
                            emd_segments, evaluate_classes)                            # Chamfer and earth mover's distances)
from . import query_eval  # noqa: F401,E402  (the 2-D evaluation: mask smoothing, IoU, localisation, masked PSNR)
from .query_eval import QueryEvaluator, frame_metrics, smooth_masks  # noqa: F401,E402
from .keyframe_seed import seed_rows  # noqa: F401,E402  (a keyframe's new Gaussians from its RGB-D image, on the device)
from .frontend import KeyframeSelector, ingest_frame, median_depth, tracking_mask  # noqa: F401,E402  (the front end's frame step)
from .slam_iterations import KeyframeWindow  # noqa: F401,E402  (mapping's bundle adjustment: window poses and exposures)
from .slam import OnlineSlam, ate_rmse, ate_statistics  # noqa: F401,E402  (the online session: RGB-D frames in, poses and a map out)
from . import map_io  # noqa: F401,E402  (the map on disk: point_cloud.ply packed on the device, the resumable .npz)
from .losses import isotropic_loss  # noqa: F401,E402  (the mapping loss's isotropic regulariser)

__all__ = ["render", "OnlineSlam", "ate_rmse", "ate_statistics", "map_io", "ingest_frame", "KeyframeWindow", "isotropic_loss", "seed_rows", "tracking_mask", "median_depth", "KeyframeSelector", "LanguageDecoder", "LanguageQuery", "LanguageEncoder", "SingleStageEncoder", "SingleStageDecoder", "SingleStageQuery", "SingleStageTargets", "HighResLanguageNet", "ClipTrunk", "TSDFVolume", "earth_mover_distance", "emd_segments",
           "chamfer_distance", "chamfer_segments", "evaluate_classes", "query_eval", "QueryEvaluator", "smooth_masks", "frame_metrics", "GaussianRasterizationSettings", "GaussianRasterizer", "LanguageGaussianRasterizer",
           "rasterize_gaussians", "rasterize_language_gaussians", "BWD_REFERENCE", "BWD_EXACT", "set_backward_mode",
           "set_tile", "BINNING_RECT", "BINNING_ELLIPSE", "set_binning"]


def set_backward_mode(mode):
    """BWD_REFERENCE (default, what the shipped reference computes) or BWD_EXACT (true gradient)."""
    from . import _C
    if mode not in (BWD_REFERENCE, BWD_EXACT):
        raise ValueError("mode must be BWD_REFERENCE or BWD_EXACT")
    _C.BWD_MODE = mode


def set_binning(binning):
    """BINNING_ELLIPSE (default): a Gaussian is listed only in the tiles its alpha >= 1/255 ellipse reaches —
    identical images and gradients, about half the instances.  BINNING_RECT: the reference's bounding-square
    lists (getRect, CR/auxiliary.h:46-56), for bit-identical num_rendered / point lists."""
    from . import _C
    if binning not in (BINNING_RECT, BINNING_ELLIPSE):
        raise ValueError("binning must be BINNING_RECT or BINNING_ELLIPSE")
    _C.BINNING = binning


def set_tile(tile):
    """Logical tile edge: 15 (reference, CR/config.h:17-18) or 16 (upstream 3DGS / MonoGS)."""
    from . import _C
    if tile not in (15, 16):
        raise ValueError("tile must be 15 or 16")
    _C.TILE = tile
