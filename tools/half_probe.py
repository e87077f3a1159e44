"""C2's workload (aeon_amd/configs.py: 256 records of 256 x 256 uint8 -> 3 x 224 x 224, crop + flip +
standardize) with float32, float16 and bfloat16 outputs in one process: the step time by device events and
the tile kernel's own time (Context.set_timing / kernel_times), the types alternating in blocks of steps.
Algorithmic bytes = every crop read once + the output written once at the element size; reported as TB/s
and as a share of the 8 TB/s HBM peak.  One JSON line per type, then a summary line.

Usage: python tools/half_probe.py [--steps 200] [--block 10] [--warmup 20]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import aeon_amd as A  # noqa: E402
from aeon_amd import configs as C  # noqa: E402

HBM_PEAK = 8.0e12
TYPES = [("float32", "float"), ("float16", "float16"), ("bfloat16", "bfloat16")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="timed steps per type and pass")
    ap.add_argument("--block", type=int, default=10, help="consecutive steps of one type")
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    batch, w, h = C.CONFIGS["C2"]["batch_size"], 256, 256
    torch.cuda.set_device(0)
    ctx = A.Context(0)
    # a source pool of 8 batches (400 MB, as bench.py's: larger than the 256 MB last-level cache), one per step in turn
    pool = 8
    src = torch.randint(0, 256, (pool * batch * w * h * 3,), dtype=torch.uint8, device="cuda")
    descs = [(A.ImgDesc * batch)(*[A.ImgDesc(offset=(k * batch + i) * w * h * 3, width=w, height=h, stride=w * 3, channels=3)
                                   for i in range(batch)]) for k in range(pool)]
    f = A.ParamFactory(C.C2_AUG)
    states = A.seed_slots(1, batch)
    # one batch of params per pool batch, the same for every type
    plist = [(A.AugParams * batch)(*[f.make_params(states[i:i + 1], w, h, 224, 224) for i in range(batch)])
             for _ in range(8)]
    crop_bytes = [sum(p.crop_w * p.crop_h * 3 for p in ps) for ps in plist]
    outs, dsts, esize = {}, {}, {}
    for name, _ in TYPES:
        esize[name] = 4 if name == "float32" else 2
        outs[name] = A.out_desc(channels=3, channel_major=True, bgr_to_rgb=True, dtype=name, mean=C.MEAN, stddev=C.STDDEV,
                                item_stride=3 * 224 * 224 * esize[name])
        dsts[name] = torch.empty(batch * outs[name].item_stride, dtype=torch.uint8, device="cuda")
    stream_obj = torch.cuda.Stream()
    torch.cuda.set_stream(stream_obj)
    stream = stream_obj.cuda_stream

    def step(name, s):
        ctx.augment_batch(descs[s % pool], src.data_ptr(), plist[s % len(plist)], outs[name], dsts[name].data_ptr(), stream)

    for s in range(args.warmup):
        for name, _ in TYPES:
            step(name, s)
    torch.cuda.synchronize()
    ctx.kernel_times()

    rounds = max(1, args.steps // args.block)
    span_ms = {n: [] for n, _ in TYPES}
    kern = {n: [0.0, 0] for n, _ in TYPES}
    nbytes = {n: 0.0 for n, _ in TYPES}
    # pass A: no per-launch timing events; one event pair around each block of back-to-back steps
    for r in range(rounds):
        for name, _ in TYPES:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            step(name, r)  # (the block's first step only fills the queue)
            e0.record(stream_obj)
            for s in range(args.block):
                step(name, r * args.block + s)
                nbytes[name] += crop_bytes[(r * args.block + s) % len(plist)] + batch * 3 * 224 * 224 * esize[name]
            e1.record(stream_obj)
            e1.synchronize()
            span_ms[name].append(e0.elapsed_time(e1) / args.block)
    # pass B: the kernel's own duration, every launch timed
    ctx.set_timing(1)
    for r in range(rounds):
        for name, _ in TYPES:
            for s in range(args.block):
                step(name, r * args.block + s)
            ctx.synchronize(stream)
            ms, _, n = ctx.kernel_times()["augment"]
            kern[name][0] += ms
            kern[name][1] += n
    ctx.set_timing(0)
    res = {}
    for name, _ in TYPES:
        steps = rounds * args.block
        step_us = float(np.mean(span_ms[name])) * 1e3
        kernel_us = kern[name][0] / max(1, kern[name][1]) * 1e3
        per_step = nbytes[name] / steps
        res[name] = {"type": name, "steps": steps, "step_us": round(step_us, 2),
                     "step_us_median": round(float(np.median(span_ms[name])) * 1e3, 2),
                     "step_us_min": round(float(np.min(span_ms[name])) * 1e3, 2),
                     "kernel_us": round(kernel_us, 2), "launches_timed": kern[name][1],
                     "algorithmic_MB_per_step": round(per_step / 1e6, 2),
                     "step_TBps": round(per_step / (step_us * 1e-6) / 1e12, 3),
                     "kernel_TBps": round(per_step / (kernel_us * 1e-6) / 1e12, 3),
                     "kernel_share_of_peak": round(per_step / (kernel_us * 1e-6) / HBM_PEAK, 3)}
        print(json.dumps(res[name]), flush=True)
    print(json.dumps({"summary": {n: [res[n]["step_us"], res[n]["kernel_us"], res[n]["kernel_share_of_peak"]]
                                  for n, _ in TYPES}, "device": torch.cuda.get_device_name(0)}))
    ctx.close()


if __name__ == "__main__":
    main()
