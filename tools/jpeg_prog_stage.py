"""Progressive JPEG rates on the GPU box: windows of 512 files through Context.decode_jpeg_batch, three ways:
  device  progressive=True: the scans on the GPU (jpeg_prog_scan level by level, jpeg_prog_mask)
  host    the same call without the flag: the scans on the context's host pool (decode_file), the parent's path
  seq     the same images re-encoded sequential, through jpeg_huff: what a progressive file costs extra
Classes: img_2112_70 and flowers (aeon's two test images, the committed fixtures at their quality) and photo256 (a
256 x 256 4:2:0 q75 photo-like image, synthetic_image).  Prints one JSON line per class and route: records/s and the
GPU time per record between the events around the call's launches (aeon_hip_kernel_times, kind "jpeg").  `--runs N`
starts N fresh processes per class and route, alternating the routes, and prints min..max."""
import argparse
import io
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.environ.get("AEON_AMD_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aeon_amd as A  # noqa: E402

ROUTES = ("device", "host", "seq")


def make_files(kind, route, n, distinct=32):
    if kind != "photo256":
        z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_fixtures.npz"))
        return [z[("" if route == "seq" else "prog_") + kind + ".jpg"].tobytes()] * n
    from PIL import Image
    out = []
    for i in range(distinct):
        b = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(A.synthetic_image(100 + i, 256, 256, 3)[:, :, ::-1]), "RGB").save(
            b, "JPEG", quality=75, subsampling=2, progressive=route != "seq")
        out.append(b.getvalue())
    return [out[i % distinct] for i in range(n)]


def run_stage(kind, route, n, windows, warmup):
    import torch
    files = make_files(kind, route, n)
    descs, off = [], 0
    for b in files:
        w, h, _ = A.jpeg_info(b)
        descs.append(A.ImgDesc(offset=off, width=w, height=h, stride=w * 3, channels=3))
        off += (w * h * 3 + 15) // 16 * 16
    assert all(A.jpeg_prog_route(b) == (route != "seq") for b in files[:32]), "a file of the class is not routed as the route says"
    dst = torch.empty(off, dtype=torch.uint8, device="cuda")
    ctx, stream = A.Context(0), torch.cuda.current_stream().cuda_stream
    jf, d = A.JpegFiles(files), (A.ImgDesc * n)(*descs)

    def window():
        ctx.decode_jpeg_batch(jf, d, dst.data_ptr(), stream, progressive=route == "device")

    for _ in range(warmup):
        window()
    ctx.synchronize(stream)
    t0 = time.perf_counter()
    for _ in range(windows):
        window()
    ctx.synchronize(stream)
    dt = time.perf_counter() - t0
    ctx.set_timing(1)
    ctx.kernel_times()
    for _ in range(4):
        window()
    ctx.synchronize(stream)
    ms, _, cnt = ctx.kernel_times()["jpeg"]
    ctx.close()
    return {"class": kind, "route": route, "records": n, "windows": windows, "file_bytes_per_record": sum(len(b) for b in files) / n,
            "records_per_s": n * windows / dt, "ms_per_window": dt / windows * 1e3, "gpu_us_per_record": ms * 1e3 / max(cnt, 1) / n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", default="img_2112_70,flowers,photo256")
    ap.add_argument("--route", default="device", choices=ROUTES)
    ap.add_argument("--records", type=int, default=512)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=0, help="fresh processes per class and route, alternating; min..max")
    a = ap.parse_args()
    for kind in a.classes.split(","):
        if not a.runs:
            print(json.dumps(run_stage(kind, a.route, a.records, a.windows, a.warmup)), flush=True)
            continue
        got = {r: [] for r in ROUTES}
        for _ in range(a.runs):
            for route in ROUTES:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--classes", kind, "--route", route, "--records", str(a.records),
                                      "--windows", str(a.windows), "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=300, check=True).stdout
                got[route].append(json.loads(out.strip().splitlines()[-1]))
        span = lambda rs, k, nd: [round(min(r[k] for r in rs), nd), round(max(r[k] for r in rs), nd)]
        print(json.dumps({"class": kind, "runs": a.runs, **{f"{r}_records_per_s": span(got[r], "records_per_s", 0) for r in ROUTES},
                          **{f"{r}_gpu_us_per_record": span(got[r], "gpu_us_per_record", 2) for r in ROUTES},
                          "device_faster_than_host_in_every_pair": all(x["records_per_s"] > y["records_per_s"] for x, y in zip(got["device"], got["host"])),
                          "host_faster_than_device_in_every_pair": all(x["records_per_s"] < y["records_per_s"] for x, y in zip(got["device"], got["host"]))}),
              flush=True)


if __name__ == "__main__":
    main()
