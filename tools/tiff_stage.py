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
  pal_lzw_tiled      the pal_lzw masks in 128 x 128 LZW tiles (tiff_convert_tiled; pal_lzw is their strip twin)
  rgb512_raw_tiled   512 x 512 RGB in 128 x 128 uncompressed tiles; rgb512_raw: the same images in strips of 5 rows
  rgb512_deflate_tiled  the same in 128 x 128 Deflate tiles with predictor 2; rgb512_deflate: in strips of 5 rows
  rgb_lzw_64k / rgb_lzw_1strip  the rgb_lzw images in Pillow's default strips (64 KB: 85 rows) and in one strip;
  pal_lzw_tiled256 / pal_packbits_tiled256  the pal_lzw masks in 256 x 256 LZW / PackBits tiles (pal_packbits_tiled: in
                  128 x 128 PackBits tiles).  Their strips and tiles are above 32 KiB: `--route large` sends them
                  through aeon_hip_decode_tiff_large_batch (tiff_expand_large); the plain device route keeps them on the host
Prints one JSON line per class: records/s, H2D bytes per record and, on the device route, the kernels' GPU time per
record (aeon_hip_kernel_times, kind "png": the PNG, pixmap and TIFF decode kernels).  `--runs N` starts N fresh
processes per class and route, alternating the routes, and prints min..max.
"""
import argparse
import io
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


def _tiff(im, compression, predictor, rows):
    info = {278: rows} if rows else {}  # (no RowsPerStrip: Pillow's default, strips of 64 KB)
    if predictor:
        info[317] = 2
    buf = io.BytesIO()
    im.save(buf, "TIFF", compression=compression, tiffinfo=info)
    return buf.getvalue()


def _tiled(a, photo, compression, predictor, tile=128, palette=None):
    """`a` (HxW or HxWxS uint8, both multiples of `tile`) as a little-endian tiled file.  Pillow writes no tiles: every
    tile is saved through it as a one-strip file, and that strip's bytes (libtiff's own LZW or Deflate) become the tile."""
    from PIL import Image
    h, w, spp = a.shape[0], a.shape[1], 1 if a.ndim == 2 else a.shape[2]
    blobs = []
    for y in range(0, h, tile):
        for x in range(0, w, tile):
            t = np.ascontiguousarray(a[y:y + tile, x:x + tile])
            if compression is None:
                blobs.append(t.tobytes())
                continue
            f = _tiff(Image.fromarray(t, "RGB" if spp == 3 else "L"), compression, predictor, tile)
            ifd = struct.unpack_from("<I", f, 4)[0]
            tags = {struct.unpack_from("<H", f, e)[0]: struct.unpack_from("<I", f, e + 8)[0]
                    for e in range(ifd + 2, ifd + 2 + 12 * struct.unpack_from("<H", f, ifd)[0], 12)}
            blobs.append(f[tags[273]:tags[273] + tags[279]])
    comp = {None: 1, "tiff_lzw": 5, "tiff_adobe_deflate": 8, "packbits": 32773}[compression]
    tags = [(256, 4, [w]), (257, 4, [h]), (258, 3, [8] * spp), (259, 3, [comp]), (262, 3, [photo]), (277, 3, [spp]),
            (317, 3, [2 if predictor else 1])] + ([(320, 3, palette)] if palette else []) + \
           [(322, 3, [tile]), (323, 3, [tile]), (324, 4, None), (325, 4, [len(b) for b in blobs])]
    body, offs = bytearray(8), []
    for b in blobs:
        offs.append(len(body))
        body += b + b"\0" * (len(b) & 1)
    ifd = struct.pack("<H", len(tags))
    for t, ty, v in tags:
        data = struct.pack("<" + "HI"[ty == 4] * len(v or offs), *(v or offs))
        if len(data) > 4:
            ifd += struct.pack("<HHII", t, ty, len(v or offs), len(body))
            body += data
        else:
            ifd += struct.pack("<HHI", t, ty, len(v or offs)) + data.ljust(4, b"\0")
    body[:8] = b"II" + struct.pack("<HI", 42, len(body))
    return bytes(body + ifd + bytes(4))


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
        if kind in ("rgb_raw", "rgb_lzw", "rgb_lzw_64k", "rgb_lzw_1strip"):
            im = Image.fromarray(np.ascontiguousarray(A.synthetic_image(100 + i, 256, 256, 3)[:, :, ::-1]), "RGB")
            rows = {"rgb_lzw_64k": None, "rgb_lzw_1strip": 256}.get(kind, 10)
            out.append(_tiff(im, None, False, 10) if kind == "rgb_raw" else _tiff(im, "tiff_lzw", True, rows))
        elif kind.startswith("pal_"):
            mask, pal = _blobs(rng, 512), [int(v) for v in rng.integers(0, 256, 768)]
            if "_tiled" in kind:  # (ColorMap: 3 x 256 shorts, plane after plane)
                out.append(_tiled(mask, 3, "packbits" if "packbits" in kind else "tiff_lzw", False, tile=256 if kind.endswith("256") else 128,
                                  palette=[257 * pal[3 * i + c] for c in range(3) for i in range(256)]))
                continue
            im = Image.fromarray(mask, "P")
            im.putpalette(pal)
            out.append(_tiff(im, "tiff_lzw", False, 16))
        elif kind.startswith("rgb512"):
            rgb = np.ascontiguousarray(A.synthetic_image(100 + i, 512, 512, 3)[:, :, ::-1])
            compression, predictor = ("tiff_adobe_deflate", True) if "deflate" in kind else (None, False)
            out.append(_tiled(rgb, 2, compression, predictor) if kind.endswith("_tiled") else
                       _tiff(Image.fromarray(rgb, "RGB"), compression, predictor, 5))
        else:
            ramp = (np.add.outer(np.arange(512), np.arange(512)) * 37 + i * 101).astype(np.uint16)
            noise = {"gray16_deflate": 64, "gray16_deflate_r3": 6, "gray16_deflate_r6": 2}[kind]
            im = Image.fromarray((ramp + rng.integers(0, noise, (512, 512)).astype(np.uint16)).astype(np.uint16))
            out.append(_tiff(im, "tiff_adobe_deflate", True, 8))
    return [out[i % distinct] for i in range(n)]


MODE = {"rgb_raw": A.DECODE_BGR8, "rgb_lzw": A.DECODE_BGR8, "pal_lzw": A.DECODE_ANYDEPTH, "gray16_deflate": A.DECODE_ANYDEPTH,
        "gray16_deflate_r3": A.DECODE_ANYDEPTH, "gray16_deflate_r6": A.DECODE_ANYDEPTH, "pal_lzw_tiled": A.DECODE_ANYDEPTH,
        "rgb512_raw": A.DECODE_BGR8, "rgb512_raw_tiled": A.DECODE_BGR8, "rgb512_deflate": A.DECODE_BGR8,
        "rgb512_deflate_tiled": A.DECODE_BGR8, "rgb_lzw_64k": A.DECODE_BGR8, "rgb_lzw_1strip": A.DECODE_BGR8,
        "pal_lzw_tiled256": A.DECODE_ANYDEPTH, "pal_packbits_tiled256": A.DECODE_ANYDEPTH, "pal_packbits_tiled": A.DECODE_ANYDEPTH}


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
    if route != "host":
        large = route == "large"
        assert all(A.tiff_large_route(b) if large else A.tiff_host_stage(b, mode)[0] for b in files[:32]), \
            "a file of the class is not routed to the device"
        res["h2d_bytes_per_record"] = sum(len(b) for b in files[:32]) / 32
        jf = A.JpegFiles(files)
        d = (A.ImgDesc * n)(*descs)
        m = (A.ctypes.c_int * n)(*([mode] * n))

        def window():
            ctx.decode_tiff_batch(jf, m, d, dst.data_ptr(), stream, large_strips=large)
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
    if route != "host":
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
    ap.add_argument("--route", default="device", choices=["device", "large", "host"],
                    help="with --runs: the device-side route of every pair (device or large), against host")
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
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--classes", kind, "--route", "large" if (route, a.route) == ("device", "large") else route,
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
