"""Scoring of the result files the inference drivers write: VIPSeg VPQ / STQ (vps.py, on the pair tables of pair_counts.py), VSPW
mIoU / VC8 / VC16 (vss.py, on the per-video counts of vss_counts.py) and DAVIS J / F (davis.py, on the per-pair counts of
davis_counts.py)."""
_DAVIS = ("DAVISEvaluator", "db_statistics", "disk_radius", "evaluate_davis_files", "jf_from_counts", "read_sequence")
__all__ = list(_DAVIS)


def __getattr__(name):                       # on first use: `python -m univs_amd.evaluation.davis` imports this package before its module
    if name in _DAVIS:
        from . import davis
        return getattr(davis, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
