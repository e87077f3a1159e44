"""PNG stage rates on the GPU box: windows of 512 PNG records through aeon_hip_decode_png_batch (the device
route: compressed bytes up, png_inflate + png_unfilter) or, `--route host`, through what a decoder without the
stage does with them (aeon_decode_png on 16 pool threads into pinned memory, one H2D of the pixels), and the C5
decoder (image + mask, both PNG) end to end.  Classes:
  photo   256 x 256 RGB photo-like images (synthetic_image), zlib level 6
  mask    512 x 512 palette masks, five classes in blobs
  depth   512 x 512 16-bit gray
  c5      Decoder over photo + mask records (C5: 512 x 512 outputs), whatever route the library takes
Prints one JSON line per class: records/s, H2D bytes per record and, on the device route, the two kernels' GPU
time per record (aeon_hip_kernel_times).  The same script runs against a parent commit's library, where only
`--route host` and c5 exist; compare fresh processes, alternating.
"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.environ.get("AEON_AMD_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aeon_amd as A  # noqa: E402
from aeon_amd import configs as C  # noqa: E402


def _png(arr, mode=None, palette=None):
    from PIL import Image
    im = Image.fromarray(arr, mode) if mode else Image.fromarray(arr)
    if palette is not None:
        im.putpalette(palette)
    buf = io.BytesIO()
    im.save(buf, "PNG", compress_level=6)
    return buf.getvalue()


def _blobs(rng, side):
    cls = rng.integers(0, 5, (side // 64, side // 64)).astype(np.uint8)
    m = np.kron(cls, np.ones((64, 64), np.uint8))
    return np.roll(m, int(rng.integers(0, 64)), axis=1)


VOC = [v for c in range(5) for v in (c * 30, c * 50, 255 - c * 40)]


def make_files(kind, n, distinct=32):
    rng = np.random.default_rng(7)
    out = []
    for i in range(distinct):
        if kind == "photo":
            out.append(_png(np.ascontiguousarray(A.synthetic_image(100 + i, 256, 256, 3)[:, :, ::-1])))
        elif kind == "mask":
            out.append(_png(_blobs(rng, 512), "P", VOC))
        else:
            ramp = (np.add.outer(np.arange(512), np.arange(512)) * 37 + i * 101).astype(np.uint16)
            out.append(_png((ramp + rng.integers(0, 64, (512, 512)).astype(np.uint16)).astype(np.uint16)))
    return [out[i % distinct] for i in range(n)]


MODE = {"photo": 0, "mask": 2, "depth": 2}


def run_stage(kind, route, n, windows, warmup):
    import torch
    files = make_files(kind, n)
    mode = MODE[kind]
    descs, off = [], 0
    for b in files:
        w, h, d, c = A.png_info(b)
        eb = 2 if (mode == 2 and d == 16 and c != 3) else 1
        cn = 3 if mode == 0 else 1
        descs.append(A.ImgDesc(offset=off, width=w, height=h, stride=w * cn * eb, channels=cn, elem_bytes=eb))
        off += (w * h * cn * eb + 15) // 16 * 16
    dst = torch.empty(off, dtype=torch.uint8, device="cuda")
    ctx = A.Context(0)
    stream = torch.cuda.current_stream().cuda_stream
    res = {"class": kind, "route": route, "records": n, "windows": windows,
           "file_bytes_per_record": sum(len(b) for b in files) / n}
    if route == "device":
        staged = [A.png_host_stage(b, mode) for b in files[:32]]
        assert all(r for r, _ in staged), "a file of the class is not routed to the device"
        res["h2d_bytes_per_record"] = sum(s for _, s in staged) / len(staged)
        jf = A.JpegFiles(files)
        d = (A.ImgDesc * n)(*descs)
        m = (A.ctypes.c_int * n)(*([mode] * n))

        def window():
            ctx.decode_png_batch(jf, m, d, dst.data_ptr(), stream)
    else:
        res["h2d_bytes_per_record"] = off / n
        pinned = torch.empty(off, dtype=torch.uint8).pin_memory()
        base = pinned.data_ptr()
        pool = ThreadPoolExecutor(16)
        lib = A.lib()

        def one(i):
            de = descs[i]
            rc = lib.aeon_decode_png(files[i], len(files[i]), mode, A.ctypes.c_void_p(base + de.offset), de.stride, None)
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
    ctx.close()
    return res


def run_c5(n, windows, warmup):
    import torch
    photos, masks = make_files("photo", n), make_files("mask", n)
    # (the mask is cut to the photo's size by using a 256 x 256 corner: image and mask of a record agree in size)
    rng = np.random.default_rng(9)
    small = [_png(_blobs(rng, 256), "P", VOC) for _ in range(32)]
    recs = [(photos[i], small[i % 32]) for i in range(n)]
    cfg = dict(batch_size=n, random_seed=3, etl=[C.IMAGE_512, C.MASK_512], augmentation=[C.C5_AUG])
    d = A.Decoder(cfg)
    enc = d.encoded(recs)
    sizes = [o["item_bytes"] * n for o in d.outputs]
    bufs = [[torch.empty(s, dtype=torch.uint8).pin_memory() for s in sizes] for _ in range(2)]

    def run(k):
        d.submit(enc, [b.data_ptr() for b in bufs[0]])
        for w in range(1, k):
            d.submit(enc, [b.data_ptr() for b in bufs[w % 2]])
            d.wait()
        d.wait()
    run(warmup)
    t0 = time.perf_counter()
    run(windows)
    dt = time.perf_counter() - t0
    route = "device" if hasattr(A, "png_host_stage") else "host"
    return {"class": "c5", "route": route, "records": n, "windows": windows, "records_per_s": n * windows / dt,
            "ms_per_window": dt / windows * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", default="photo,mask,depth,c5")
    ap.add_argument("--route", default="device", choices=["device", "host"])
    ap.add_argument("--records", type=int, default=512)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    for kind in a.classes.split(","):
        r = run_c5(a.records, a.windows, a.warmup) if kind == "c5" else run_stage(kind, a.route, a.records, a.windows, a.warmup)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
