"""Scoring of the result files the inference drivers write (VIPSeg VPQ / STQ: vps.py, on the pair tables of pair_counts.py)."""
