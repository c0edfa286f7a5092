"""Frames from disk to the drivers, test mode only: the records of a video annotation file or of a folder of frames (datasets.py), of
a video-object-segmentation file with its first-frame masks (vos_datasets.py), `read_image` (images.py), the test-time mappers
(mapper.py, vos_mapper.py) and the integer rules of their resizes (resize_rule.py); the records of a VOS data set in its own folders of frames and annotation PNGs (vos_folders.py) and the
numpy statement of the prompts made from those PNGs' id maps (idmap_rule.py); the records of a folder of images or of a panoptic
annotation file with its class table (image_datasets.py) and the per-image test mapper (image_mapper.py)."""
from .datasets import load_video_json, video_records_from_dir
from .image_datasets import class_table, image_records_from_dir, load_categories_json, load_panoptic_json
from .image_mapper import ImageTestMapper
from .images import read_image, read_images
from .mapper import VideoTestMapper, resize_params_from_config
from .resize_rule import nearest_table, resize_nearest, resize_tables, resize_u8_reference, shortest_edge_size
from .vos_datasets import is_vos_name, load_vos_json
from .vos_folders import vos_records_from_dirs
from .vos_mapper import VOSTestMapper

__all__ = ["load_video_json", "video_records_from_dir", "read_image", "read_images", "VideoTestMapper", "resize_params_from_config", "resize_tables",
           "resize_u8_reference", "shortest_edge_size", "nearest_table", "resize_nearest", "is_vos_name", "load_vos_json", "VOSTestMapper", "vos_records_from_dirs",
           "image_records_from_dir", "load_panoptic_json", "load_categories_json", "class_table", "ImageTestMapper"]
