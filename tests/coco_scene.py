"""A seeded COCO-format scene for the mask-AP tests: polygon ground truth, RLE results, and the same scene as a one-frame YouTube-VIS file."""
import functools

import numpy as np

from univs_amd.data import polygon_rule as rule

SIZES = {1: (40, 50), 2: (33, 47), 3: (64, 64), 4: (21, 90), 5: (48, 36), 6: (30, 30)}


def counts_of(polygons, h, w):
    """Uncompressed RLE counts of an object by the literal rule."""
    b = rule.object_runs(polygons, h, w)
    return [int(v) for v in np.diff([0] + b)]


def _blob(rng, h, w):
    k = int(rng.integers(3, 8))
    cx, cy, r = rng.uniform(0.15 * w, 0.85 * w), rng.uniform(0.15 * h, 0.85 * h), rng.uniform(2.0, 0.4 * min(h, w))
    t = np.sort(rng.uniform(0, 2 * np.pi, k))
    rad = r * rng.uniform(0.6, 1.0, k)
    return np.round(np.stack([cx + rad * np.cos(t), cy + rad * np.sin(t)], 1), 2).reshape(-1).tolist()


@functools.lru_cache(maxsize=None)
def scene(seed=5, crowd=False):
    """-> (gt dataset with polygon segmentations, results with uncompressed-RLE segmentations)."""
    rng = np.random.default_rng(seed)
    images = [{"id": i, "height": h, "width": w, "file_name": f"{i:06d}.jpg"} for i, (h, w) in SIZES.items()]
    cats = [{"id": 3, "name": "cat"}, {"id": 7, "name": "dog"}, {"id": 9, "name": "cup"}]
    anns, results = [], []
    for im in images:
        h, w = im["height"], im["width"]
        for _ in range(int(rng.integers(0, 6)) if im["id"] != 6 else 0):          # image 6: detections only
            polys = [_blob(rng, h, w) for _ in range(int(rng.integers(1, 3)))]
            c = counts_of(polys, h, w)
            area = int(sum(c[1::2]))
            if area == 0:
                continue
            cat = int(rng.choice([3, 7, 9]))
            anns.append({"id": len(anns) + 1, "image_id": im["id"], "category_id": cat, "segmentation": polys, "area": area, "iscrowd": 0})
            if rng.uniform() < 0.8:                                                 # a detection near it: the polygon, jittered
                jit = [(np.asarray(p) + rng.normal(0, 0.8, len(p))).round(2).tolist() for p in polys]
                results.append({"image_id": im["id"], "category_id": cat if rng.uniform() < 0.9 else 3,
                                "segmentation": {"size": [h, w], "counts": counts_of(jit, h, w)}, "score": float(np.round(rng.uniform(0.2, 1.0), 1))})
        for _ in range(int(rng.integers(0, 4))):                                    # detections of nothing
            results.append({"image_id": im["id"], "category_id": int(rng.choice([3, 7, 9])),
                            "segmentation": {"size": [h, w], "counts": counts_of([_blob(rng, h, w)], h, w)}, "score": float(np.round(rng.uniform(0.1, 0.9), 1))})
    if crowd:
        h, w = SIZES[1]
        c = counts_of([[2.0, 2.0, 30.0, 2.0, 30.0, 30.0, 2.0, 30.0]], h, w)
        anns.append({"id": len(anns) + 1, "image_id": 1, "category_id": 9, "segmentation": {"size": [h, w], "counts": c}, "area": 784, "iscrowd": 1})
    order = rng.permutation(len(results))
    return ({"images": images, "annotations": anns, "categories": cats}, [results[i] for i in order])


def with_rle_ground_truth(dataset):
    """The same data set, every polygon segmentation as uncompressed RLE."""
    sizes = {im["id"]: (im["height"], im["width"]) for im in dataset["images"]}
    anns = []
    for a in dataset["annotations"]:
        a = dict(a)
        if isinstance(a["segmentation"], list):
            h, w = sizes[a["image_id"]]
            a["segmentation"] = {"size": [h, w], "counts": counts_of(a["segmentation"], h, w)}
        anns.append(a)
    return dict(dataset, annotations=anns)


def as_ytvis(dataset, results):
    """The crowd-free scene as a YouTube-VIS file of one-frame videos and its result records."""
    rle = with_rle_ground_truth(dataset)
    videos = [{"id": im["id"], "height": im["height"], "width": im["width"], "length": 1} for im in dataset["images"]]
    anns = [{"id": a["id"], "video_id": a["image_id"], "category_id": a["category_id"], "segmentations": [a["segmentation"]],
             "areas": [a["area"]], "iscrowd": 0} for a in rle["annotations"]]
    res = [{"video_id": r["image_id"], "category_id": r["category_id"], "segmentations": [r["segmentation"]], "score": r["score"]} for r in results]
    return {"videos": videos, "annotations": anns, "categories": dataset["categories"]}, res
