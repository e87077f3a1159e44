"""What the box targets cost a decode window: windows of 256 synthetic 300x300 records with 8 boxes each
through the decoder's device-output path, [image] alone and [localization_ssd, image] with the same
augmentation, each window bracketed by HIP events on its stream (the call returns when the window is
complete, so the bracket is the window: draw + extract, staging, H2D, kernels).  Warm-up windows, then
--windows timed ones; prints one JSON line with both medians and their difference.

    python tools/box_window_timing.py [--records 256] [--windows 30] [--warmup 5]

Under `rocprofv3 --kernel-trace --stats -- python tools/box_window_timing.py` the kernel statistics give
the box kernel's own time (box_targets).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import aeon_amd as A  # noqa: E402

CLASSES = ["a", "b", "c", "d"]
AUG = {"type": "image", "crop_enable": False, "flip_enable": True, "expand_ratio": [1.0, 4.0],
       "expand_probability": 0.5,
       "batch_samplers": [{"max_sample": 1, "max_trials": 50, "sampler": {"scale": [0.3, 1.0], "aspect_ratio": [0.5, 2.0]},
                           "sample_constraint": {"min_jaccard_overlap": 0.1}}, {"max_trials": 1}]}
IMAGE = {"type": "image", "height": 300, "width": 300, "channels": 3, "output_type": "float", "channel_major": True}
SSD = {"type": "localization_ssd", "height": 300, "width": 300, "max_gt_boxes": 64, "class_names": CLASSES}


def records(n):
    rng = np.random.default_rng(1)
    recs = []
    for i in range(n):
        img = A.synthetic_image(i % 32, 300, 300, 3)
        objs = []
        for _ in range(8):
            x0, y0 = int(rng.integers(0, 250)), int(rng.integers(0, 250))
            objs.append({"bndbox": {"xmin": x0, "ymin": y0, "xmax": x0 + int(rng.integers(10, 49)),
                                    "ymax": y0 + int(rng.integers(10, 49))},
                         "name": CLASSES[int(rng.integers(0, 4))], "difficult": False})
        meta = json.dumps({"object": objs, "size": {"width": 300, "height": 300, "depth": 3}}).encode()
        recs.append((meta, img))
    return recs


def time_windows(etl, recs, windows, warmup):
    import torch
    d = A.Decoder(dict(batch_size=len(recs), random_seed=7, etl=etl, augmentation=[AUG]))
    enc = d.encoded(recs)
    bufs = [torch.zeros(len(recs) * o["item_bytes"], dtype=torch.uint8, device="cuda") for o in d.outputs]
    ptrs = (ctypes.c_void_p * len(bufs))(*[t.data_ptr() for t in bufs])
    stream = torch.cuda.current_stream()
    ms = []
    for k in range(warmup + windows):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        A._check_host(A.lib().aeon_decoder_decode_encoded(d._h, len(recs), enc.elems, ptrs, 1,
                                                          ctypes.c_void_p(stream.cuda_stream)))
        end.record(stream)
        end.synchronize()
        if k >= warmup:
            ms.append(start.elapsed_time(end))
    d.close()
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=256)
    ap.add_argument("--windows", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    recs = records(a.records)
    img = time_windows([IMAGE], [(r[1],) for r in recs], a.windows, a.warmup)
    ssd = time_windows([SSD, IMAGE], recs, a.windows, a.warmup)
    print(json.dumps({"records": a.records, "windows": a.windows, "image_ms_median": img[0], "image_ms_min_max": img[1:],
                      "ssd_image_ms_median": ssd[0], "ssd_image_ms_min_max": ssd[1:],
                      "difference_ms": ssd[0] - img[0]}))


if __name__ == "__main__":
    main()
