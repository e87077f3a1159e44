"""What the localization_rcnn targets kernel costs a decode window at aeon's own test shape: 1000 x 1000
(34 596 anchors), 256 records of 6 boxes each, through aeon_hip_rcnn_targets_batch into device buffers.
Every element of every output is written, 12 x total_anchors 32-bit words per record (1.66 MB; 425 MB
for the window), so next to the time the tool reports the store bandwidth that time amounts to.

Two measurements, each after warm-up calls:
  * shuffle off (aeon's debug_deterministic): the calls are asynchronous, so `--calls` launches run back to
    back between one pair of HIP events; time per call = elapsed / calls (it includes the call's table H2D,
    a few KB, and whatever of the host's part of a call the GPU had to wait for);
  * shuffle on: a call hands the engines' end states back and synchronizes, so each call is bracketed by
    its own pair of events (the host's part of the call, table H2D, kernel, the states' D2H); the median is
    reported.  One wave per record runs std::shuffle's draws over the record's foreground and background
    lists, which is most of the difference between the two numbers.

    python tools/rcnn_window_timing.py [--records 256] [--boxes 6] [--calls 20] [--warmup 3]

prints one JSON line.  Under `rocprofv3 --kernel-trace --stats -- python tools/rcnn_window_timing.py` the
kernel statistics give the kernel's own time (rcnn_targets).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import aeon_amd as A  # noqa: E402

CFG = {"type": "localization_rcnn", "height": 1000, "width": 1000, "class_names": ["a", "b", "c", "d"]}
SRC_W, SRC_H, SCALE = 500, 375, 1.6  # aeon's loader test: a 500 x 375 image at fixed_scaling_factor 1.6


def records(n, boxes):
    rng = np.random.default_rng(1)
    recs = []
    for _ in range(n):
        x0, y0 = rng.integers(0, SRC_W - 120, boxes), rng.integers(0, SRC_H - 120, boxes)
        b = np.stack([x0, y0, x0 + rng.integers(30, 120, boxes), y0 + rng.integers(30, 120, boxes)], 1).astype(np.float32)
        recs.append((b, rng.integers(0, 4, boxes).astype(np.int32), np.zeros(boxes, np.int32)))
    return recs


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=256)
    ap.add_argument("--boxes", type=int, default=6)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    n = a.records
    recs = records(n, a.boxes)
    p = A.aug_params(crop_x=0, crop_y=0, crop_w=SRC_W, crop_h=SRC_H, out_w=int(SRC_W * SCALE), out_h=int(SRC_H * SCALE),
                     flip=0, expand_ratio=1.0)
    params = (A.AugParams * n)(*[p] * n)
    ctx = A.Context(0)
    prepared = A.RcnnCall(ctx, CFG, recs, params, fixed_scaling_factor=SCALE)  # the C call alone is timed
    prepared.out.anchors_key = 1  # the context's one anchor table, named as the decoder's provider names its own
    A_ = int(prepared.info["total_anchors"])
    bufs = [torch.zeros(n * s, dtype=torch.uint8, device="cuda") for s in prepared.strides]
    ptrs = [t.data_ptr() for t in bufs]
    stream = torch.cuda.current_stream()
    sid = stream.cuda_stream
    states = A.seed_slots(7, n)

    def call(shuffle):
        prepared.launch(ptrs, states if shuffle else None, shuffle, sid)

    for _ in range(a.warmup):
        call(False)
    ctx.synchronize(sid)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(stream)
    for _ in range(a.calls):
        call(False)
    end.record(stream)
    end.synchronize()
    off_ms = start.elapsed_time(end) / a.calls
    sampled = int(bufs[3].cpu().numpy().view(np.int32).sum()) // 2
    for _ in range(a.warmup):
        call(True)
    on = []
    for _ in range(a.calls):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        call(True)
        end.record(stream)
        end.synchronize()
        on.append(start.elapsed_time(end))
    ctx.close()
    window_bytes = 12 * A_ * 4 * n
    on_ms = float(np.median(on))
    print(json.dumps({"records": n, "boxes_per_record": a.boxes, "total_anchors": A_, "calls": a.calls,
                      "window_mb": window_bytes / 1e6, "sampled_anchors_per_record": sampled / n,
                      "shuffle_off_ms_per_window": off_ms, "shuffle_off_store_gb_s": window_bytes / off_ms / 1e6,
                      "shuffle_on_ms_median": on_ms, "shuffle_on_ms_min_max": [float(min(on)), float(max(on))],
                      "shuffle_on_store_gb_s": window_bytes / on_ms / 1e6}))


if __name__ == "__main__":
    main()
