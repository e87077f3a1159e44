"""Records, configurations and comparisons the decoder tests of the box providers (tests/test_hip_boxes.py,
tests/test_hip_rcnn.py) share: synthetic images with random object boxes and their JSON metadata, the image and
localization_ssd ETL objects with the SSD augmentation (tests/test_ssd.py draws over it too), and the ssd
reference over tests/box_ref.py."""
import json

import numpy as np

import aeon_amd as A
from aeon_amd import configs as CFG
from tests import box_ref as B
from tests import helpers as H

CLASSES = ["cat", "dog", "bird"]
SIDE = 128
SSD_ETL = {"type": "localization_ssd", "height": SIDE, "width": SIDE, "max_gt_boxes": 4, "class_names": CLASSES}
IMG_ETL = {"type": "image", "height": SIDE, "width": SIDE, "channels": 3, "output_type": "float",
           "channel_major": True}
SSD_AUG = {"type": "image", "crop_enable": False, "flip_enable": True, "expand_ratio": [1.0, 4.0],
           "expand_probability": 0.5, "brightness": [0.875, 1.125], "saturation": [0.5, 1.5],
           "batch_samplers": [
               {"max_sample": 1, "max_trials": 50,
                "sampler": {"scale": [0.3, 1.0], "aspect_ratio": [0.5, 2.0]},
                "sample_constraint": {"min_jaccard_overlap": 0.1}},
               {"max_sample": 1, "max_trials": 50,
                "sampler": {"scale": [0.3, 1.0], "aspect_ratio": [0.5, 2.0]},
                "sample_constraint": {"min_object_coverage": 0.5, "max_sample_coverage": 0.9}},
               {"max_trials": 1}]}


def random_boxes(rng, w, h, n):
    res = []
    for _ in range(n):
        x0, y0 = float(rng.integers(0, w - 1)), float(rng.integers(0, h - 1))
        res.append((x0, y0, float(rng.integers(int(x0), w)), float(rng.integers(int(y0), h))))
    return res


def meta_json(w, h, boxes, labels, difficult):
    objs = [{"bndbox": {"xmin": b[0], "ymin": b[1], "xmax": b[2], "ymax": b[3]}, "name": CLASSES[l],
             "difficult": bool(d)} for b, l, d in zip(boxes, labels, difficult)]
    return json.dumps({"object": objs, "size": {"width": w, "height": h, "depth": 3}}).encode()


def box_window(n, seed):
    """n records of 96..160 px synthetic images with 0..6 boxes each."""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        w, h = int(rng.integers(96, 161)), int(rng.integers(96, 161))
        k = int(rng.integers(0, 7))
        boxes = random_boxes(rng, w, h, k)
        recs.append(dict(img=A.synthetic_image(1000 * seed + i, w, h, 3), w=w, h=h, boxes=boxes,
                         labels=rng.integers(0, 3, k).tolist(), difficult=rng.integers(0, 2, k).tolist()))
    return recs


def as_records(recs):
    """(metadata, image) per record: the elements of a [box provider, image] configuration."""
    return [(meta_json(r["w"], r["h"], r["boxes"], r["labels"], r["difficult"]), r["img"]) for r in recs]


def ssd_reference(recs, f, states, aug, etl_img=IMG_ETL, ssd=SSD_ETL):
    """The five localization_ssd outputs (box_ref over make_ssd_params on the slot engines, in record order
    through one factory) and the oracle's image records for the same params."""
    params = [f.make_ssd_params(states[i:i + 1], r["w"], r["h"], ssd["width"], ssd["height"], r["boxes"])
              for i, r in enumerate(recs)]
    want = [B.load_ssd(r["boxes"], r["labels"], r["difficult"], p, ssd["max_gt_boxes"], ssd["width"], ssd["height"],
                       f.emit()) for r, p in zip(recs, params)]
    out = {k: np.stack([np.asarray(w[k]) for w in want]) for k in A.SSD_OUTPUTS}
    out["image"] = np.stack(H.oracle_records([r["img"] for r in recs], params, CFG.out_desc_for(etl_img, aug)))
    return out, params


def assert_outputs(got, want, what):
    for k, w in want.items():
        g = np.asarray(got[k]).reshape(w.shape)
        assert np.array_equal(g.view(np.uint32) if g.dtype.itemsize == 4 else g,
                              w.view(np.uint32) if w.dtype.itemsize == 4 else w), (what, k)
