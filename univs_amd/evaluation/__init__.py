"""Scoring of the result files the inference drivers write: VIPSeg VPQ / STQ (vps.py, on the pair tables of pair_counts.py), VSPW
mIoU / VC8 / VC16 (vss.py, on the per-video counts of vss_counts.py) and DAVIS J / F (davis.py, on the per-pair counts of
davis_counts.py) and YouTube-VIS AP / AR (ytvis.py, on the per-video overlap counts of vis_counts.py) and VIPOSeg panoptic-VOS mask /
boundary IoU (pvos.py, on the per-id counts of pvos_counts.py) and HOTA of YouTube-VIS-format tracking results (hota.py, on the per-video
tables of hota_counts.py) and PQ / mIoU of per-image results (image.py, on pair_counts at one frame and the confusion count of
imagelabels_ops.py) and COCO instance mask AP of per-image results (coco.py, on the polygon rasteriser of polygon_ops.py and the
overlap counts of vis_counts.py at one frame)."""
_DAVIS = ("DAVISEvaluator", "db_statistics", "disk_radius", "evaluate_davis_files", "jf_from_counts", "read_sequence")
_YTVIS = ("YTVISEval", "YTVISEvaluator", "derive_coco_results", "evaluate_predictions_on_ytvis", "load_results")
_VIS_COUNTS = ("Runs", "runs_from_rles", "vis_overlap", "vis_overlap_aten", "vis_video_overlap")
_PVOS = ("PVOSEvaluator", "evaluate_pvos_files")
_PVOS_COUNTS = ("dilation", "pvos_counts_aten", "pvos_video_counts")      # (`pvos_counts` itself is the module of that name)
_HOTA = ("HOTAEvaluator", "evaluate_hota_files", "hota_from_idmaps")
_HOTA_COUNTS = ("HotaTables", "hota_counts_aten", "hota_video_counts", "lsa_max")      # (`hota_counts` itself is the module of that name)
_IMAGE = ("PanopticEvaluator", "SemSegEvaluator", "evaluate_panoptic_files", "evaluate_semseg_files", "semseg_scores")
_COCO = ("COCOInstanceEvaluator", "COCOSegmEval", "evaluate_predictions_on_coco")
__all__ = list(_DAVIS + _YTVIS + _VIS_COUNTS + _PVOS + _PVOS_COUNTS + _HOTA + _HOTA_COUNTS + _IMAGE + _COCO)


def __getattr__(name):                       # on first use: `python -m univs_amd.evaluation.davis` imports this package before its module
    if name in _DAVIS:
        from . import davis
        return getattr(davis, name)
    if name in _YTVIS:
        from . import ytvis
        return getattr(ytvis, name)
    if name in _VIS_COUNTS:
        from . import vis_counts
        return getattr(vis_counts, name)
    if name in _PVOS:
        from . import pvos
        return getattr(pvos, name)
    if name in _PVOS_COUNTS:
        from . import pvos_counts
        return getattr(pvos_counts, name)
    if name in _HOTA:
        from . import hota
        return getattr(hota, name)
    if name in _HOTA_COUNTS:
        from . import hota_counts
        return getattr(hota_counts, name)
    if name in _IMAGE:
        from . import image
        return getattr(image, name)
    if name in _COCO:
        from . import coco
        return getattr(coco, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
