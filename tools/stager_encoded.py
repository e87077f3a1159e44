"""The aeon-side drop-in fed encoded records, measured.

Writes the two JPEG files bench.py's run_e2e_jpeg decodes (aeon's img_2112_70.jpg 480x360 and flowers.jpg 600x800,
tests/golden/jpeg_fixtures.npz) to a scratch directory with a list file naming them, and runs
aeon_amd/aeon_path_cpp (tools/aeon_path_cpp.cpp) on C2 with post_process launch-only ("overlap"), for pinned and for
pageable batch buffers, each in fresh processes that alternate, `--pairs` times:
  encoded     provide() = aeon_encoded_info + make_params + aeon_hip_stager_stage_encoded of the file
  pixels      provide() = make_params + aeon_hip_stager_stage of a decoded record of the file's size
  today       the tool without a list: decoded 256x256 synthetic records, the README's aeon-path figure
and the project's own Decoder (aeon_decoder_submit / wait, pinned host outputs) on the same files and window size,
also in a fresh process per run.  None of the stager runs pays for cv::imdecode: `pixels` and `today` leave it out,
`encoded` replaces it.  Prints one JSON object: per case min .. max images/s and every run, and the bytes that
cross PCIe host-to-device per record.

usage: python tools/stager_encoded.py [--pairs 3] [--windows 24] [--warmup 4]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXE = os.path.join(ROOT, "aeon_amd", "aeon_path_cpp")


def run_tool(buffers, windows, warmup, *tail):
    r = subprocess.run([EXE, "C2", buffers, "overlap", str(windows), str(warmup), "256", *tail], capture_output=True,
                       text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(f"aeon_path_cpp {buffers} {tail}: {r.stderr.strip()[-300:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def decoder_rate(batch, windows):
    """One run of the project's own front door on the same files (bench.py's run_e2e_jpeg, host outputs)."""
    import torch

    import aeon_amd as A
    import bench
    from aeon_amd import configs as C
    return bench.run_e2e_jpeg(A, C, torch, batch=batch, windows=windows, on_device=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--windows", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--decoder-only", type=int, default=0, help="(internal) print the Decoder's rate for this window size")
    args = ap.parse_args()
    if args.decoder_only:
        print(json.dumps({"value": decoder_rate(args.decoder_only, args.windows)}))
        return
    import aeon_amd as A
    import bench
    files = bench.jpeg_files(2)
    res = {"files": [], "runs": {}, "h2d_bytes_per_record": {}}
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i, f in enumerate(files):
            paths.append(os.path.join(tmp, f"record{i}.jpg"))
            with open(paths[-1], "wb") as fh:
                fh.write(f)
            info = A.encoded_info(f)
            gpu, staged = A.jpeg_host_stage(f)
            res["files"].append(dict(bytes=len(f), width=info["width"], height=info["height"], gpu_entropy=gpu,
                                     staged_bytes=staged))
        lst = os.path.join(tmp, "records.txt")
        with open(lst, "w") as fh:
            fh.write("\n".join(paths) + "\n")
        decode_size = None
        for buffers in ("pinned", "pageable"):
            for _ in range(args.pairs):
                for case, tail in (("encoded", (lst,)), ("pixels", (lst, "pixels")), ("today", ())):
                    d = run_tool(buffers, args.windows, args.warmup, *tail)
                    decode_size = d["decode_size"]
                    res["runs"].setdefault(f"{case}/{buffers}", []).append(round(d["value"]))
                    if tail:  # the decode thread's time per window: container wait, provide(), post_process
                        res.setdefault("decode_thread_ms", {}).setdefault(f"{case}/{buffers}", []).append(
                            [d["container_wait_ms"], d["provide_ms"], d["post_process_ms"], d["ms_per_window"]])
                    if case == "encoded":
                        res["encoded_report"] = {k: d[k] for k in ("device_decoded", "host_decoded", "staged_pixels",
                                                                   "src_zero_copy", "decode_size", "pool_threads")}
                if buffers == "pinned":  # the Decoder's host outputs are pinned
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--decoder-only", str(decode_size),
                                        "--windows", str(args.windows)], capture_output=True, text=True, timeout=300)
                    if r.returncode != 0:
                        raise RuntimeError(f"decoder run: {r.stderr.strip()[-300:]}")
                    res["runs"].setdefault("decoder/pinned", []).append(round(json.loads(r.stdout.strip().splitlines()[-1])["value"]))
    n = len(res["files"])
    staged = sum(f["staged_bytes"] for f in res["files"]) / n
    res["h2d_bytes_per_record"] = {"encoded": staged, "decoder": staged,
                                   "pixels": sum(f["width"] * f["height"] * 3 for f in res["files"]) / n,
                                   "today": 256 * 256 * 3}
    res["min_max"] = {k: [min(v), max(v)] for k, v in res["runs"].items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
