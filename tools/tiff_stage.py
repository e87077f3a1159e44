"""TIFF stage rates on the GPU box: windows of 512 TIFF records through aeon_hip_decode_tiff_batch (the device
route: the files up as they are, tiff_expand and tiff_convert) or, `--route host`, through what a decoder without the
stage does with them (aeon_decode_tiff on 16 pool threads into pinned memory, one H2D of the pixels; separate host
code, not the kernels under test).  Classes:
  rgb_raw         256 x 256 RGB, uncompressed (photo-like, synthetic_image), decoded to BGR8
  rgb_lzw         the same images, LZW + predictor 2
  pal_lzw         512 x 512 8-bit palette masks, LZW, decoded at ANYDEPTH (the gray of the palette entry)
  gray16_deflate  512 x 512 16-bit gray (depth-like: a ramp with 6 bits of noise), Deflate + predictor 2, decoded at
                  ANYDEPTH; gray16_deflate_r3 / _r6 (not in the default list): the same with less noise, streams a third
                  and a sixth or less of the samples, for the crossover of the decoder's routing rule
Prints one JSON line per class: records/s, H2D bytes per record and, on the device route, the kernels' GPU time per
record (aeon_hip_kernel_times, kind "png": the PNG, pixmap and TIFF decode kernels).  `--runs N` starts N fresh
processes per class and route, alternating the routes, and prints min..max.
"""
import argparse
import io
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.environ.get("AEON_AMD_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aeon_amd as A  # noqa: E402


def _tiff(im, compression, predictor, rows):
    info = {278: rows}
    if predictor:
        info[317] = 2
    buf = io.BytesIO()
    im.save(buf, "TIFF", compression=compression, tiffinfo=info)
    return buf.getvalue()


def _blobs(rng, side):
    cls = rng.integers(0, 5, (side // 64, side // 64)).astype(np.uint8)
    return np.roll(np.kron(cls, np.ones((64, 64), np.uint8)), int(rng.integers(0, 64)), axis=1)


def make_files(kind, n, distinct=32):
    """Written by Pillow (libtiff), in strips of libtiff's own default size, about 8 KB decoded each (Pillow's default
    of 64 KB a strip would keep the LZW classes on the host route)."""
    from PIL import Image
    rng = np.random.default_rng(7)
    out = []
    for i in range(distinct):
        if kind in ("rgb_raw", "rgb_lzw"):
            im = Image.fromarray(np.ascontiguousarray(A.synthetic_image(100 + i, 256, 256, 3)[:, :, ::-1]), "RGB")
            out.append(_tiff(im, None, False, 10) if kind == "rgb_raw" else _tiff(im, "tiff_lzw", True, 10))
        elif kind == "pal_lzw":
            im = Image.fromarray(_blobs(rng, 512), "P")
            im.putpalette([int(v) for v in rng.integers(0, 256, 768)])
            out.append(_tiff(im, "tiff_lzw", False, 16))
        else:
            ramp = (np.add.outer(np.arange(512), np.arange(512)) * 37 + i * 101).astype(np.uint16)
            noise = {"gray16_deflate": 64, "gray16_deflate_r3": 6, "gray16_deflate_r6": 2}[kind]
            im = Image.fromarray((ramp + rng.integers(0, noise, (512, 512)).astype(np.uint16)).astype(np.uint16))
            out.append(_tiff(im, "tiff_adobe_deflate", True, 8))
    return [out[i % distinct] for i in range(n)]


MODE = {"rgb_raw": A.DECODE_BGR8, "rgb_lzw": A.DECODE_BGR8, "pal_lzw": A.DECODE_ANYDEPTH, "gray16_deflate": A.DECODE_ANYDEPTH,
        "gray16_deflate_r3": A.DECODE_ANYDEPTH, "gray16_deflate_r6": A.DECODE_ANYDEPTH}


def run_stage(kind, route, n, windows, warmup):
    import torch
    files = make_files(kind, n)
    mode = MODE[kind]
    descs, off = [], 0
    for b in files:
        w, h, _, eb2 = A.tiff_info(b)
        eb = eb2 if mode == A.DECODE_ANYDEPTH else 1
        cn = 3 if mode == A.DECODE_BGR8 else 1
        descs.append(A.ImgDesc(offset=off, width=w, height=h, stride=w * cn * eb, channels=cn, elem_bytes=eb))
        off += (w * h * cn * eb + 15) // 16 * 16
    dst = torch.empty(off, dtype=torch.uint8, device="cuda")
    ctx = A.Context(0)
    stream = torch.cuda.current_stream().cuda_stream
    res = {"class": kind, "route": route, "records": n, "windows": windows,
           "file_bytes_per_record": sum(len(b) for b in files) / n, "record_bytes": off / n}
    if route == "device":
        staged = [A.tiff_host_stage(b, mode) for b in files[:32]]
        assert all(r for r, _ in staged), "a file of the class is not routed to the device"
        res["h2d_bytes_per_record"] = sum(s for _, s in staged) / len(staged)
        jf = A.JpegFiles(files)
        d = (A.ImgDesc * n)(*descs)
        m = (A.ctypes.c_int * n)(*([mode] * n))

        def window():
            ctx.decode_tiff_batch(jf, m, d, dst.data_ptr(), stream)
    else:
        res["h2d_bytes_per_record"] = off / n
        pinned = torch.empty(off, dtype=torch.uint8).pin_memory()
        base = pinned.data_ptr()
        pool = ThreadPoolExecutor(16)
        lib = A.lib()

        def one(i):
            de = descs[i]
            rc = lib.aeon_decode_tiff(files[i], len(files[i]), mode, A.ctypes.c_void_p(base + de.offset), de.stride, None)
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
    ap.add_argument("--classes", default="rgb_raw,rgb_lzw,pal_lzw,gray16_deflate")
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
