"""Pixmap stage rates on the GPU box: windows of 512 BMP / PNM records through aeon_hip_decode_pixmap_batch (the
device route: the files up as they are, pixmap_convert) or, `--route host`, through what a decoder without the
stage does with them (aeon_decode_pixmap on 16 pool threads into pinned memory, one H2D of the pixels; separate host
code, not the kernel under test).  Classes:
  p6      256 x 256 P6 (photo-like, synthetic_image), decoded to BGR8
  p5w     512 x 512 16-bit P5 (depth-like), decoded at ANYDEPTH
  bmp8    512 x 512 8-bit palette BMP masks, decoded at ANYDEPTH (the gray of the palette entry)
  p4      512 x 512 P4 bitmaps, decoded to GRAY8
Prints one JSON line per class: records/s, H2D bytes per record and, on the device route, the kernel's GPU time per
record (aeon_hip_kernel_times, kind "png": the PNG and pixmap decode kernels).  `--runs N` starts N fresh processes
per class and route, alternating the routes, and prints min..max.
"""
import argparse
import json
import os
import struct
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.environ.get("AEON_AMD_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aeon_amd as A  # noqa: E402


def _pnm(magic, a, maxval):
    h, w = a.shape[:2]
    head = b"P%d\n%d %d\n" % (magic, w, h) + (b"" if magic == 4 else b"%d\n" % maxval)
    if magic == 4:
        return head + np.packbits(a.astype(bool), axis=1).tobytes()
    return head + (a.astype(">u2") if maxval > 255 else a.astype(np.uint8)).tobytes()


def _bmp8(idx, palette):
    h, w = idx.shape
    pitch = (w + 3) & ~3
    rows = np.zeros((h, pitch), np.uint8)
    rows[:, :w] = idx[::-1]
    pal = np.concatenate([palette, np.zeros((256, 1), np.uint8)], 1).tobytes()
    off = 14 + 40 + len(pal)
    info = struct.pack("<IiiHHIIiiII", 40, w, h, 1, 8, 0, pitch * h, 2835, 2835, 0, 0)
    return b"BM" + struct.pack("<IHHI", off + pitch * h, 0, 0, off) + info + pal + rows.tobytes()


def _blobs(rng, side):
    cls = rng.integers(0, 5, (side // 64, side // 64)).astype(np.uint8)
    return np.roll(np.kron(cls, np.ones((64, 64), np.uint8)), int(rng.integers(0, 64)), axis=1)


def make_files(kind, n, distinct=32):
    rng = np.random.default_rng(7)
    out = []
    for i in range(distinct):
        if kind == "p6":
            out.append(_pnm(6, A.synthetic_image(100 + i, 256, 256, 3)[:, :, ::-1], 255))
        elif kind == "p5w":
            ramp = (np.add.outer(np.arange(512), np.arange(512)) * 37 + i * 101).astype(np.uint16)
            out.append(_pnm(5, (ramp + rng.integers(0, 64, (512, 512)).astype(np.uint16)).astype(np.uint16), 65535))
        elif kind == "bmp8":
            out.append(_bmp8(_blobs(rng, 512), rng.integers(0, 256, (256, 3)).astype(np.uint8)))
        else:
            out.append(_pnm(4, _blobs(rng, 512) & 1, 1))
    return [out[i % distinct] for i in range(n)]


MODE = {"p6": A.DECODE_BGR8, "p5w": A.DECODE_ANYDEPTH, "bmp8": A.DECODE_ANYDEPTH, "p4": A.DECODE_GRAY8}


def run_stage(kind, route, n, windows, warmup):
    import torch
    files = make_files(kind, n)
    mode = MODE[kind]
    descs, off = [], 0
    for b in files:
        w, h, d, _, _ = A.pixmap_info(b)
        eb = 2 if (mode == A.DECODE_ANYDEPTH and d == 16) else 1
        cn = 3 if mode == A.DECODE_BGR8 else 1
        descs.append(A.ImgDesc(offset=off, width=w, height=h, stride=w * cn * eb, channels=cn, elem_bytes=eb))
        off += (w * h * cn * eb + 15) // 16 * 16
    dst = torch.empty(off, dtype=torch.uint8, device="cuda")
    ctx = A.Context(0)
    stream = torch.cuda.current_stream().cuda_stream
    res = {"class": kind, "route": route, "records": n, "windows": windows,
           "file_bytes_per_record": sum(len(b) for b in files) / n, "record_bytes": off / n}
    if route == "device":
        staged = [A.pixmap_host_stage(b, mode) for b in files[:32]]
        assert all(r for r, _ in staged), "a file of the class is not routed to the device"
        res["h2d_bytes_per_record"] = sum(s for _, s in staged) / len(staged)
        jf = A.JpegFiles(files)
        d = (A.ImgDesc * n)(*descs)
        m = (A.ctypes.c_int * n)(*([mode] * n))

        def window():
            ctx.decode_pixmap_batch(jf, m, d, dst.data_ptr(), stream)
    else:
        res["h2d_bytes_per_record"] = off / n
        pinned = torch.empty(off, dtype=torch.uint8).pin_memory()
        base = pinned.data_ptr()
        pool = ThreadPoolExecutor(16)
        lib = A.lib()

        def one(i):
            de = descs[i]
            rc = lib.aeon_decode_pixmap(files[i], len(files[i]), mode, A.ctypes.c_void_p(base + de.offset), de.stride, None)
            assert rc == 0

        def window():
            list(pool.map(one, range(n), chunksize=8))
            dst.copy_(pinned, non_blocking=True)
    for _ in range(warmup):
        window()
    ctx.synchronize(stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(windows):
        window()
    ctx.synchronize(stream)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res["records_per_s"] = n * windows / dt
    res["ms_per_window"] = dt / windows * 1e3
    if route == "device":
        ctx.set_timing(1)
        ctx.kernel_times()
        for _ in range(4):
            window()
        ctx.synchronize(stream)
        ms, by, cnt = ctx.kernel_times()["png"]
        ctx.set_timing(0)
        res["kernel_us_per_record"] = ms * 1e3 / max(cnt, 1) / n
        res["kernel_gb_per_s"] = by / max(ms, 1e-9) / 1e6
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", default="p6,p5w,bmp8,p4")
    ap.add_argument("--route", default="device", choices=["device", "host"])
    ap.add_argument("--records", type=int, default=512)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=0, help="fresh processes per class and route, alternating; min..max")
    a = ap.parse_args()
    if not a.runs:
        for kind in a.classes.split(","):
            print(json.dumps(run_stage(kind, a.route, a.records, a.windows, a.warmup)), flush=True)
        return
    for kind in a.classes.split(","):
        got = {"device": [], "host": []}
        for _ in range(a.runs):
            for route in ("device", "host"):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--classes", kind, "--route", route,
                                      "--records", str(a.records), "--windows", str(a.windows), "--warmup", str(a.warmup)],
                                     capture_output=True, text=True, timeout=300, check=True).stdout
                got[route].append(json.loads(out.strip().splitlines()[-1]))
        dev, host = got["device"], got["host"]
        rate = lambda rs: [round(min(r["records_per_s"] for r in rs)), round(max(r["records_per_s"] for r in rs))]
        print(json.dumps({"class": kind, "runs": a.runs, "device_records_per_s": rate(dev), "host_records_per_s": rate(host),
                          "device_faster_in_every_pair": all(d["records_per_s"] > h["records_per_s"] for d, h in zip(dev, host)),
                          "host_faster_in_every_pair": all(d["records_per_s"] < h["records_per_s"] for d, h in zip(dev, host)),
                          "device_h2d_bytes_per_record": dev[0]["h2d_bytes_per_record"],
                          "host_h2d_bytes_per_record": host[0]["h2d_bytes_per_record"],
                          "kernel_us_per_record": [round(min(r["kernel_us_per_record"] for r in dev), 3),
                                                   round(max(r["kernel_us_per_record"] for r in dev), 3)],
                          "kernel_gb_per_s": [round(min(r["kernel_gb_per_s"] for r in dev)), round(max(r["kernel_gb_per_s"] for r in dev))]}),
              flush=True)


if __name__ == "__main__":
    main()
