"""The TIFF files of the stage's tests (tests/test_tiff_stage.py on the CPU, tests/test_hip_tiff.py on the GPU), made
by tests/tiff_writer.py: device_files() are routed to the device, host_files() stay with the host decoder.  The
shapes are the smallest at which the kernels can go wrong: widths 1-9, 15-17, 63-65, 255-257 (the dword groups of a
row, the scan's chunk of 64 pixels, the workgroup's 256 lanes), heights 1, 2, 3, 65, RowsPerStrip 1, 2, h and a
value that does not divide h, every alignment 0..15 of the first strip, rows wider than a band (16 KiB of source:
2,100 RGBA16 and 5,500 RGB pixels, the only shapes above 512 a side), strips of exactly 32,768 and 32,769 decoded
bytes, and the LZW / PackBits / Deflate streams a common encoder does not write.
"""
import functools
import zlib

import numpy as np

from tests import tiff_writer as W

WIDTHS = list(range(1, 10)) + [15, 16, 17, 63, 64, 65, 255, 256, 257]
HEIGHTS = [1, 2, 3, 65]
COMPS = ["raw", "lzw", "packbits", "deflate"]
# (name, samples per pixel, dtype, photometric, ExtraSamples)
KINDS = [("gray8", 1, np.uint8, 1, None), ("rgb8", 3, np.uint8, 2, None), ("gray16", 1, np.uint16, 1, None),
         ("rgba8", 4, np.uint8, 2, 1), ("rgb16", 3, np.uint16, 2, None), ("pal8", 1, np.uint8, 3, None),
         ("white8", 1, np.uint8, 0, None), ("ga16", 2, np.uint16, 1, 0), ("white16", 1, np.uint16, 0, None),
         ("rgbx16", 4, np.uint16, 2, None), ("pala8", 2, np.uint8, 3, 1)]


def image(rng, h, w, spp, dtype, noise=8):
    """Smooth ramps with runs and a little noise: LZW and Deflate find matches, PackBits finds both run classes."""
    top = 65536 if dtype == np.uint16 else 256
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([(x * (3 + c) * (top // 256) // 2 + y * 5 * (top // 256) + c * 40) % top for c in range(spp)], axis=2)
    a = a + rng.integers(0, noise + 1, a.shape) * (rng.random(a.shape) < 0.3)
    a[:, w // 3: w // 3 + max(2, w // 4)] = a[:, w // 3: w // 3 + 1]  # a flat run in every row
    return (a % top).astype(dtype)


def colormap(rng):
    return rng.integers(0, 65536, (256, 3)).astype(np.uint16)


def make(rng, kind, h, w, comp, **kw):
    name, spp, dtype, photo, extra = kind
    a = image(rng, h, w, spp, dtype)
    if photo == 3:
        kw.setdefault("colormap", colormap(rng))
        kw["pred"] = 1
    return W.write(a, photo, comp, extra=extra, **kw)


@functools.lru_cache(None)
def device_files():
    rng = np.random.default_rng(21)
    out, k = [], 0
    for w in WIDTHS:
        for h in HEIGHTS:
            kind, comp = KINDS[k % len(KINDS)], COMPS[(k // 2) % 4]
            rps = [1, 2, None, h, h // 2 + 1][k % 5]
            rowb = w * kind[1] * np.dtype(kind[2]).itemsize
            if comp in ("lzw", "packbits") and (rps or h) * rowb > 32768:
                rps = 32768 // rowb  # (the device's strip cap)
            f = make(rng, kind, h, w, comp, big=bool(k % 3 == 1), pred=1 + (k % 4 == 2 or k % 7 == 0), rps=rps, pad=k % 16,
                     ifd_first=bool(k % 6 == 5))
            out.append((f"{kind[0]}_{w}x{h}_{comp}_rps{rps}_{k}", f))
            k += 1
    for pad in range(16):  # every alignment of the first strip, each compression
        for comp in COMPS:
            kind = KINDS[(pad + COMPS.index(comp)) % len(KINDS)]
            out.append((f"align{pad}_{comp}", make(rng, kind, 5, 13, comp, pad=pad, rps=2, pred=1 + pad % 2, big=bool(pad & 4))))
    # a row wider than a band: walked in pieces, the predictor's sums carried across them
    for comp, big, rps in [("raw", False, 1), ("lzw", True, 1), ("deflate", True, 2)]:
        out.append((f"wide_{comp}", make(rng, KINDS[9], 2, 2100, comp, pred=2, big=big, rps=rps)))
    out.append(("wide_rgb8_pred", make(rng, KINDS[1], 1, 5500, "packbits", pred=2, rps=1)))
    # strips of exactly 32,768 decoded bytes (the device's cap)
    for comp in ("lzw", "packbits"):
        out.append((f"cap32768_{comp}", make(rng, KINDS[0], 128, 512, comp, rps=64)))
    # LZW streams
    noise = rng.integers(0, 256, (1, 5600)).astype(np.uint8)
    out.append(("lzw_table_full", W.write(noise, 1, "lzw", rps=1, codec=lambda d: W.lzw(d, fill=True)[0])))
    out.append(("lzw_widths", W.write(noise, 1, "lzw", rps=1)))
    runs = np.repeat(rng.integers(0, 4, (6, 40)), 7, axis=1).astype(np.uint8)  # aaaaaaa...: KwKwK
    out.append(("lzw_kwkwk", W.write(runs, 1, "lzw", rps=3)))
    out.append(("lzw_flat", W.write(np.full((9, 300), 7, np.uint8), 1, "lzw", rps=4)))
    out.append(("lzw_clear_mid", W.write(runs, 1, "lzw", rps=6, codec=lambda d: W.lzw(d, clear_at=(1, 100, 101, 900))[0])))
    out.append(("lzw_no_eoi", W.write(runs, 1, "lzw", rps=2, codec=lambda d: W.lzw(d, eoi=False)[0])))
    out.append(("lzw_cut", W.write(runs, 1, "lzw", rps=2, tail=bytes(range(200)))))
    # PackBits: literals and repeats of 1 / 2 .. 128, the no-op byte
    pb = np.concatenate([np.arange(300) % 251, np.full(300, 9), rng.integers(0, 256, 129), np.full(128, 3), [1, 2, 2, 3, 3, 3]])
    pb = np.tile(pb.astype(np.uint8), (3, 1))
    out.append(("packbits_classes", W.write(pb, 1, "packbits", rps=2, codec=lambda d: W.packbits([d[i:i + pb.shape[1]] for i in range(0, len(d), pb.shape[1])], noop_every=3))))
    out.append(("packbits_more", W.write(pb, 1, "packbits", rps=1, tail=b"\x05\x05\x07")))
    # Deflate by hand, and streams that hold more than the strip's rows
    img = image(rng, 7, 90, 3, np.uint8)
    out.append(("deflate_stored", W.write(img, 2, "adobe", rps=3, codec=lambda d: W.deflate_stored(d, 500))))
    out.append(("deflate_fixed", W.write(runs, 1, "deflate", rps=4, codec=W.deflate_fixed)))
    out.append(("deflate_cut", W.write(img, 2, "deflate", rps=2, tail=bytes(range(256)) * 3)))
    out.append(("deflate_stored_cut", W.write(img, 2, "deflate", rps=7, tail=b"abc" * 50, codec=lambda d: W.deflate_stored(d, 700))))
    out.append(("deflate_fixed_cut", W.write(runs, 1, "deflate", rps=6, tail=b"\x09" * 300, codec=W.deflate_fixed)))
    out.append(("deflate_big_strip", make(rng, KINDS[4], 200, 300, "deflate", pred=2, rps=None)))  # 360,000 bytes, one wave
    # header forms
    out.append(("no_bytecounts", W.write(img, 2, "raw", bytecounts=False)))
    out.append(("rps_above_h", W.write(img, 2, "lzw", rps=1000)))
    out.append(("orientation", W.write(img, 2, "raw", more_tags=[(274, 3, [2])])))
    return out


@functools.lru_cache(None)
def corrupt_files():
    """Device-routed files whose header is sound and whose strip data is not: the host decoder refuses them while it
    decodes, the device reports them through the stream's error word.  Corrupt data, nothing that faults: every
    decoder checks what it reads and writes against the strip."""
    rng = np.random.default_rng(23)
    img = image(rng, 40, 60, 3, np.uint8)

    def patched(f, at, new):
        return f[:at] + new + f[at + len(new):]

    lz = W.write(img, 2, "lzw", rps=40)  # one strip right behind the header
    z = W.write(img, 2, "deflate", rps=40)
    nz = len(zlib.compress(img.tobytes(), 6))
    return [("lzw_code_above_table", patched(lz, 8 + 20, b"\xff\xff\xff")),
            ("lzw_eoi_early", W.write(img, 2, "lzw", rps=40, codec=lambda d: W.lzw(d[:len(d) // 2])[0])),
            ("deflate_adler", patched(z, 8 + nz - 1, bytes([z[8 + nz - 1] ^ 0x55]))),
            ("deflate_bad_block", patched(z, 8 + 2, b"\x07")),  # block type 3
            ("packbits_short", W.write(img, 2, "packbits", rps=40, codec=lambda d: W.packbits([d[:-5]])))]


@functools.lru_cache(None)
def host_files():
    rng = np.random.default_rng(22)
    return [(f"cap32769_{comp}", make(rng, KINDS[0], 198, 331, comp, rps=99)) for comp in ("lzw", "packbits")]
