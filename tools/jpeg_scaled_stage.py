"""The JPEG stage at scales 1, 2, 4, 8 (Context.decode_jpeg_batch(scale=...)) on a window of one fixture, and JPEG ->
C2 (224x224) with the source decoded at the largest scale that keeps both of its sides >= 224:

  stage_ms     GPU ms per window of the decode call (HIP events around its Huffman, IDCT and colour launches)
  bytes        the window's records in the source arena
  e2e_gpu_ms   decode call + C2 augment call on one stream: GPU ms per window (both calls' kernel timers)
  e2e_wall_ms  the same pair, wall time per window with the calls back to back (host work included)

Each figure is the median of `--rounds` rounds of `--calls` calls, with the rounds' lowest and highest (the run-to-run
spread).  --parent DIR loads the aeon_amd package of another checkout (one built at the parent commit) into the same
process under another name and measures it, whole-size, in rounds that alternate with this checkout's."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def load_package(root, name):
    d = os.path.join(os.path.abspath(root), "aeon_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class Window:
    """A window of `files` at 1 / scale through package A: the decode call, and the decode + C2 augment pair."""

    def __init__(self, A, ctx, files, scale):
        from aeon_amd import configs as C
        self.A, self.ctx, n = A, ctx, len(files)
        w, h, _ = A.jpeg_info(files[0])
        w, h = -(-w // scale), -(-h // scale)
        descs, off = [], 0
        for _ in files:
            descs.append(A.ImgDesc(offset=off, width=w, height=h, stride=w * 3, channels=3))
            off += (w * h * 3 + 15) // 16 * 16
        self.descs, self.bytes = (A.ImgDesc * n)(*descs), off
        self.arena = torch.empty(off, dtype=torch.uint8, device="cuda")
        self.stream = torch.cuda.Stream().cuda_stream
        self.jf, self.kw = A.JpegFiles(files), ({"scale": scale} if scale > 1 else {})
        f, states = A.ParamFactory(C.C2_AUG), A.seed_slots(1, n)
        self.params = [f.make_params(states[i:i + 1].copy(), w, h, 224, 224) for i in range(n)]
        self.out = A.out_desc(channels=3, channel_major=True, bgr_to_rgb=True, dtype="float32", mean=C.MEAN,
                              stddev=C.STDDEV, item_stride=3 * 224 * 224 * 4)
        self.dst = torch.empty(n * self.out.item_stride, dtype=torch.uint8, device="cuda")

    def run(self, calls, augment):
        """(GPU ms per window from the kernel timers, wall ms per window)."""
        ctx = self.ctx

        def once():
            ctx.decode_jpeg_batch(self.jf, self.descs, self.arena.data_ptr(), self.stream, **self.kw)
            if augment:
                ctx.augment_batch(self.descs, self.arena.data_ptr(), self.params, self.out, self.dst.data_ptr(), self.stream)
        for _ in range(4):
            once()
        ctx.synchronize(self.stream)
        t0 = time.perf_counter()
        for _ in range(calls):
            once()
        ctx.synchronize(self.stream)
        wall = (time.perf_counter() - t0) * 1e3 / calls
        ctx.kernel_times()
        ctx.set_timing(1)
        for _ in range(calls):
            once()
        ctx.synchronize(self.stream)
        t = ctx.kernel_times()
        ctx.set_timing(False)
        return sum(t[k][0] for k in ("jpeg", "augment", "pre")) / calls, wall


def spread(v):
    v = sorted(v)
    return [round(statistics.median(v), 4), round(v[0], 4), round(v[-1], 4)]  # median, lowest, highest


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import aeon_amd
    torch.cuda.set_device(0)
    sides = {"this": aeon_amd}
    if args.parent:
        sides["parent"] = load_package(args.parent, "aeon_amd_parent")
    ctxs = {k: A.Context(0) for k, A in sides.items()}
    fx = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_fixtures.npz"))
    for name in ("img_2112_70.jpg", "flowers.jpg"):
        files = [fx[name].tobytes()] * args.batch
        w, h, _ = aeon_amd.jpeg_info(files[0])
        best = max(s for s in (1, 2, 4, 8) if -(-w // s) >= 224 and -(-h // s) >= 224)
        cases = [("this", s) for s in (1, 2, 4, 8)] + ([("parent", 1)] if args.parent else [])
        wins = {c: Window(sides[c[0]], ctxs[c[0]], files, c[1]) for c in cases}
        res = {c: {"stage_ms": [], "e2e_gpu_ms": [], "e2e_wall_ms": []} for c in cases}
        for _ in range(args.rounds):  # (the sides and scales alternate inside a round)
            for c in cases:
                res[c]["stage_ms"].append(wins[c].run(args.calls, False)[0])
                if c[1] in (1, best):
                    g, wall = wins[c].run(args.calls, True)
                    res[c]["e2e_gpu_ms"].append(g), res[c]["e2e_wall_ms"].append(wall)
        for c in cases:
            print(json.dumps(dict({"side": c[0], "file": name, "size": [w, h], "scale": c[1], "bytes": wins[c].bytes},
                                  **{k: spread(v) for k, v in res[c].items() if v})), flush=True)
    for c in ctxs.values():
        c.close()
