"""A C3D decode window (128 clips x 16 frames of 171x128, 4:2:0 at quality 88 -> 3 x 16 x 112 x
112, frame augmentation scale [0.875, 0.875]) through the aeon-side stager for provider::video, against the project's
own Decoder on the same clips with a (video, label) config.

  clip     aeon_hip_stager_stage_clip: provide() hands over the AVI, the window's launch decodes its frames
  frames   aeon_hip_stager_stage_frames: provide() hands over the 16 decoded frames (aeon's video::extractor keeps
           running on the host; its cv::imdecode is NOT timed here: the frames are decoded once, before the clock)
  decoder  Decoder.submit / wait, two windows in flight

Each with pinned, pageable and device batch buffers.  The stager cases are double-buffered as aeon's two containers
are: window k+1 is staged (from --threads staging threads, each taking a slice of the window's clips) and launched
before the consumer waits for window k by buffer alone.  The cases alternate in one process, --pairs times over; a
case's figure is clips/s over --windows windows after --warmup.  The staging loop is Python over ctypes (the GIL is
released inside the calls), so the stager's figures carry that loop; the Decoder's pool is C++.

    python tools/stager_clips.py [--clips 128] [--pairs 3] [--windows 12] [--warmup 3] [--threads 14]

Prints one JSON line: per case the runs' clips/s (min, median, max) and frames/s, and the H2D bytes per clip of the
two forms (clip: what the JPEG stage stages for the clip's frames, aeon_jpeg_host_stage; frames: the decoded frames)."""
import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import aeon_amd as A  # noqa: E402
from video_window_timing import D, FRAME_AUG, OUT, SRC_H, SRC_W, pictures  # noqa: E402

ITEM = 3 * D * OUT * OUT


def avi_of(frames, width, height):
    """A plain MJPEG AVI (hdrl / avih with the index flag, one vids / MJPG strl, movi, idx1) over JPEG files."""
    import struct

    def chunk(cc, payload):
        return cc + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")

    def lst(kind, payload):
        return b"LIST" + struct.pack("<I", 4 + len(payload)) + kind + payload
    n = len(frames)
    avih = struct.pack("<14I", 40000, 0, 0, 0x10, n, 0, 1, 0, width, height, 0, 0, 0, 0)
    strh = struct.pack("<4s4s10I4h", b"vids", b"MJPG", 0, 0, 0, 1, 25, 0, n, 0, 0, 0, 0, 0, width, height)
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    movi, idx = b"", b""
    for f in frames:
        idx += struct.pack("<4sIII", b"00dc", 0x10, 4 + len(movi), len(f))
        movi += chunk(b"00dc", f)
    body = lst(b"hdrl", chunk(b"avih", avih) + lst(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf)))
    body += lst(b"movi", movi) + chunk(b"idx1", idx)
    return b"RIFF" + struct.pack("<I", 4 + len(body)) + b"AVI " + body


class Out:
    """n items of `item` bytes: pinned and mapped, pageable, or device memory."""

    def __init__(self, nbytes, where):
        import torch
        self.where = where
        if where == "device":
            self.keep = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
            self.ptr = self.keep.data_ptr()
        elif where == "pinned":
            p = ctypes.c_void_p()
            A._check(A.lib().aeon_hip_host_alloc(nbytes, ctypes.byref(p)))
            self.ptr = p.value
        else:
            self.keep = np.zeros(nbytes, np.uint8)
            self.ptr = self.keep.ctypes.data

    def free(self):
        if self.where == "pinned":
            A.lib().aeon_hip_host_free(ctypes.c_void_p(self.ptr))


def run_stager(ctx, form, where, clips, params, a, pool):
    n, L = len(clips), A.lib()
    st = A.Stager.video(ctx, D, OUT, OUT, ITEM, n, device_out=where == "device")
    bufs = [Out(n * ITEM, where) for _ in range(2)]
    if form == "clip":
        def stage(buf, i):
            return L.aeon_hip_stager_stage_clip(st._h, buf, i, clips[i], len(clips[i]), ctypes.byref(params[i]))
    else:
        ptrs = [(ctypes.c_void_p * D)(*[f.ctypes.data for f in c]) for c in clips]

        def stage(buf, i):
            return L.aeon_hip_stager_stage_frames(st._h, buf, i, D, ptrs[i], SRC_W, SRC_H, SRC_W * 3, ctypes.byref(params[i]))

    def part(buf, t):  # one staging thread's slice of the window
        for i in range(t, n, a.threads):
            A._check_stager(stage(buf, i))
    try:
        t0 = None
        for win in range(a.warmup + a.windows):
            if win == a.warmup:
                t0 = time.perf_counter()
            buf = ctypes.c_void_p(bufs[win % 2].ptr)
            list(pool.map(lambda t: part(buf, t), range(a.threads)))
            st.launch(buf.value)
            if win > 0:
                A.Stager.wait_buffer(bufs[(win - 1) % 2].ptr)
        A.Stager.wait_buffer(bufs[(a.warmup + a.windows - 1) % 2].ptr)
        dt = time.perf_counter() - t0
        info = st.last_launch()
    finally:
        st.close()
        for b in bufs:
            b.free()
    return n * a.windows / dt, info


def run_decoder(where, avis, a):
    n = len(avis)
    etl = [{"type": "video", "max_frame_count": D, "frame": {"type": "image", "height": OUT, "width": OUT}},
           {"type": "label", "binary": False}]
    d = A.Decoder(dict(batch_size=n, random_seed=7, etl=etl, augmentation=[{"type": "image", "frame": FRAME_AUG}]))
    outs = [[Out(n * o["item_bytes"], where) for o in d.outputs] for _ in range(2)]
    enc = d.encoded([(v, str(i % 101)) for i, v in enumerate(avis)])
    try:
        t0 = None
        for win in range(a.warmup + a.windows):
            if win == a.warmup:
                t0 = time.perf_counter()
            d.submit(enc, [o.ptr for o in outs[win % 2]], on_device=where == "device")
            if win > 0:
                d.wait()
        d.wait()
        dt = time.perf_counter() - t0
    finally:
        d.close()
        for os_ in outs:
            for o in os_:
                o.free()
    return n * a.windows / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=128)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--windows", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=14)
    a = ap.parse_args()
    import oracle as O
    n = a.clips
    pics = pictures(32)
    decoded = [O.jpeg_decode(f, 3) for f in pics]  # (before the clock: aeon's host decode is not part of any figure)
    staged = [A.jpeg_host_stage(f)[1] for f in pics]
    order = [[(7 * (i * D + k)) % 32 for k in range(D)] for i in range(n)]
    avis = [avi_of([pics[j] for j in o], SRC_W, SRC_H) for o in order]
    frames = [[decoded[j] for j in o] for o in order]
    f = A.ParamFactory(FRAME_AUG)
    states = A.seed_slots(7, n)
    params = [f.make_params(states[i:i + 1], SRC_W, SRC_H, OUT, OUT) for i in range(n)]
    ctx = A.Context(0)
    res = {"clips": n, "frames_per_clip": D, "pairs": a.pairs, "windows": a.windows, "threads": a.threads,
           "h2d_bytes_per_clip": {"clip": float(np.mean([sum(staged[j] for j in o) for o in order])),
                                  "frames": D * SRC_W * SRC_H * 3},
           "avi_bytes_per_clip": float(np.mean([len(v) for v in avis])), "host_imdecode_timed": False}
    runs, infos = {}, {}
    with ThreadPoolExecutor(max_workers=a.threads) as pool:
        for _ in range(a.pairs):
            for where in ("pinned", "pageable", "device"):
                for form, recs in (("clip", avis), ("frames", frames)):
                    rate, info = run_stager(ctx, form, where, recs, params, a, pool)
                    runs.setdefault(f"stager_{form}_{where}", []).append(rate)
                    infos[f"stager_{form}_{where}"] = {k: info[k] for k in ("src_zero_copy", "out_direct", "chunks")}
                runs.setdefault(f"decoder_{where}", []).append(run_decoder(where, avis, a))
    res["clips_per_s"] = {k: {"min": min(v), "median": float(np.median(v)), "max": max(v), "runs": v} for k, v in runs.items()}
    res["frames_per_s_median"] = {k: float(np.median(v)) * D for k, v in runs.items()}
    res["paths"] = infos
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
