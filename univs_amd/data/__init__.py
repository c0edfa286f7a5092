"""Frames from disk to the drivers, test mode only: the records of a video annotation file or of a folder of frames (datasets.py),
`read_image` (images.py), the test-time mapper (mapper.py) and the integer rule of its resize (resize_rule.py)."""
from .datasets import load_video_json, video_records_from_dir
from .images import read_image
from .mapper import VideoTestMapper, resize_params_from_config
from .resize_rule import resize_tables, resize_u8_reference, shortest_edge_size

__all__ = ["load_video_json", "video_records_from_dir", "read_image", "VideoTestMapper", "resize_params_from_config", "resize_tables",
           "resize_u8_reference", "shortest_edge_size"]
