"""What a C3D decode window costs on the device (aeon doc/source/provider_video.rst:89-104: etl (video, label),
16 frames of 171x128 -> 112x112, batch 128): 128 synthetic clips x 16 Pillow-encoded frames with the frame
augmentation scale [0.875, 0.875], each piece bracketed by HIP events on its stream, medians over --repeats
after --warmup:

  jpeg_ms        the JPEG stage: the window's 2,048 frames through aeon_hip_decode_jpeg_batch, 512 files a call
                 (the bracket holds the calls' host halves too: headers, unstuffing, the H2D)
  video_ms       the frame transform: aeon_hip_video_batch over the 2,048 decoded frames, every clip full
  yardstick_ms   the same 2,048 frames as 2,048 independent records of aeon_hip_augment_batch with a uint8
                 planar out desc (what the frames cost without a clip around them), min / max over its repeats
  short_ms       aeon_hip_video_batch with every second clip 8 frames long (1,536 frames + clip_pad)
  clip_pad_ms    clip_pad alone: the short variant's 192 regions of 8 frames (19.3 MB of zeros) as a call of
                 64 clips of 8 frames with no frame kept

    python tools/video_window_timing.py [--clips 128] [--repeats 30] [--warmup 5]

Prints one JSON line."""
import argparse
import ctypes
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import aeon_amd as A  # noqa: E402

SRC_W, SRC_H, OUT, D = 171, 128, 112, 16
FRAME_AUG = {"type": "image", "scale": [0.875, 0.875]}


def pictures(k):
    """k distinct JPEG files of 171x128 (4:2:0, quality 88): smooth colour with some texture."""
    from PIL import Image
    files = []
    y, x = np.mgrid[0:SRC_H, 0:SRC_W].astype(np.float32)
    for i in range(k):
        rng = np.random.default_rng(i)
        img = np.stack([127 + 120 * np.sin((x + 3 * i) / (5 + i % 3)), 127 + 120 * np.cos((y - i) / 7), (x * y + 31 * i) % 255], -1)
        img = np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(img, "RGB").save(buf, "JPEG", quality=88, subsampling=2)
        files.append(buf.getvalue())
    return files


def timed(stream, fn, repeats, warmup):
    import torch
    ms = []
    for k in range(warmup + repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        fn()
        end.record(stream)
        end.synchronize()
        if k >= warmup:
            ms.append(start.elapsed_time(end))
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    n, total = a.clips, a.clips * D
    ctx = A.Context(0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    pics = pictures(32)
    frame_bytes = SRC_W * SRC_H * 3  # a multiple of 16
    descs = (A.ImgDesc * total)(*[A.ImgDesc(offset=k * frame_bytes, width=SRC_W, height=SRC_H, stride=SRC_W * 3, channels=3)
                                  for k in range(total)])
    src = torch.zeros(total * frame_bytes, dtype=torch.uint8, device="cuda")
    calls = []
    for f in range(0, total, 512):
        m = min(512, total - f)
        calls.append((A.JpegFiles([pics[(7 * k) % 32] for k in range(f, f + m)]), (A.ImgDesc * m)(*descs[f:f + m])))

    def jpeg():
        for files, d in calls:
            ctx.decode_jpeg_batch(files, d, src.data_ptr(), sp)

    res = {"clips": n, "frames": total, "repeats": a.repeats, "jpeg_ms": timed(stream, jpeg, a.repeats, a.warmup)}
    ctx.synchronize(sp)
    f = A.ParamFactory(FRAME_AUG)
    states = A.seed_slots(7, n)
    clip_params = [f.make_params(states[i:i + 1], SRC_W, SRC_H, OUT, OUT) for i in range(n)]
    cp = (A.AugParams * n)(*clip_params)
    fp = (A.AugParams * total)(*[clip_params[k // D] for k in range(total)])
    hw = OUT * OUT
    item = 3 * D * hw
    dst = torch.zeros(n * item, dtype=torch.uint8, device="cuda")
    flat = A.out_desc(channels=3, channel_major=True, dtype="uint8", item_stride=3 * hw)
    counts = lambda c: (ctypes.c_int32 * len(c))(*c)  # noqa: E731  (marshalled once, like descs and params)
    full, short = counts([D] * n), counts([D if i % 2 == 0 else D // 2 for i in range(n)])
    none = counts([0] * (n // 2))
    # the two calls of the comparison alternate, so a drift of the clocks meets both
    v, y = [], []
    for _ in range(3):
        v.append(timed(stream, lambda: ctx.video_batch(full, descs, src.data_ptr(), cp, D, OUT, OUT, dst.data_ptr(), item, sp),
                       a.repeats // 3, a.warmup))
        y.append(timed(stream, lambda: ctx.augment_batch(descs, src.data_ptr(), fp, flat, dst.data_ptr(), sp),
                       a.repeats // 3, a.warmup))
    for key, runs in (("video_ms", v), ("yardstick_ms", y)):
        res[key] = {"median": float(np.median([r["median"] for r in runs])), "min": min(r["min"] for r in runs),
                    "max": max(r["max"] for r in runs), "run_medians": [r["median"] for r in runs]}
    res["short_ms"] = timed(stream, lambda: ctx.video_batch(short, descs, src.data_ptr(), cp, D, OUT, OUT, dst.data_ptr(), item,
                                                           sp), a.repeats, a.warmup)
    res["clip_pad_ms"] = timed(stream, lambda: ctx.video_batch(none, descs, src.data_ptr(), cp, D // 2, OUT, OUT, dst.data_ptr(),
                                                              item // 2, sp), a.repeats, a.warmup)
    res["clip_pad_bytes"] = (n // 2) * 3 * (D // 2) * hw
    ctx.synchronize(sp)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
