"""Scoring of the result files the inference drivers write: VIPSeg VPQ / STQ (vps.py, on the pair tables of pair_counts.py) and VSPW
mIoU / VC8 / VC16 (vss.py, on the per-video counts of vss_counts.py)."""
