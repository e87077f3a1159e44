"""The files of tests/test_tiff_large.py (CPU) and tests/test_hip_tiff_large.py (GPU): LZW / PackBits strips and tiles above
32 KiB, which only the opt-in call decodes on the device (tiff_expand_large).  files(): (name, file,
the pixels it was cut from, photometric, what the writer's own code stream must show).  The window is 16 KiB, so the
strips are 2 x 16,384 + 1 and + 17 and 3 x 16,384 + 3 bytes; a strip of 16,384 + 1 lies below the cap, in tiff_expand's
table by the routing rule, and is here the second strip of `both_kernels`.
"""
import functools

import numpy as np

from tests import test_tiff_tiles as T
from tests import tiff_cases as TC
from tests import tiff_ref as R
from tests import tiff_writer as W


def walk(f):
    """The code stream the writer gave the file's first strip, read back: (code, batch lane, string length) of every
    code.  Lanes as tiff_expand_large deals them where no window ends and the table is not full: the code behind a
    ClearCode is read alone (lane -1), then 64 codes a batch, a new batch behind every ClearCode."""
    tags = R.parse(f)[1]
    bits = np.unpackbits(np.frombuffer(f[tags[273][0]:tags[273][0] + tags[279][0]], np.uint8))
    at, nxt, lane, prev, lens, out = 0, 258, -1, 0, {}, []
    while True:
        width = 9 + (nxt >= 511) + (nxt >= 1023) + (nxt >= 2047)
        if at + width > len(bits):
            return out
        code, at = int(bits[at:at + width] @ (1 << np.arange(width - 1, -1, -1))), at + width
        n = 0 if code in (256, 257) else 1 if code < 256 else lens.get(code, prev + 1)
        out.append((code, lane, n))
        if code == 257:
            return out
        if code == 256:
            nxt, lane, prev, lens = 258, -1, 0, {}
            continue
        if prev and nxt < 4096:
            lens[nxt], nxt = prev + 1, nxt + 1
        lane, prev = (lane + 1) % 64, n


@functools.lru_cache(None)
def files():
    rng = np.random.default_rng(31)
    _lanes = lambda f, code: {lane for c, lane, _ in walk(f) if c == code}
    _crosses = lambda f, need: (lambda ends: need not in ends and ends[-1] > need)(np.cumsum([n for _, _, n in walk(f)]))
    gray = lambda h, w: TC.image(rng, h, w, 1, np.uint8)
    noise = rng.integers(0, 256, (200, 200, 1)).astype(np.uint8)  # 40,000 bytes: no window ends within 130 of its end
    flat = np.full((200, 250, 1), 7, np.uint8)
    lzw = lambda a, **kw: W.write(a, 1, "lzw", codec=lambda d: W.lzw(d, **kw)[0])
    out = [(f"{c}_32769", W.write(a, 1, c), a, 1, None) for c in ("lzw", "packbits") for a in [gray(99, 331)]]
    a, b = gray(395, 83), gray(580, 113)  # 32,785 bytes; strips of 49,155 and 16,385 bytes
    out += [("lzw_2chunks_17", W.write(a, 1, "lzw"), a, 1, None), ("both_kernels", W.write(b, 1, "lzw", rps=435), b, 1, None)]
    out.append(("lzw_flat", W.write(flat, 1, "lzw"), flat, 1,  # every code the one about to be defined: KwKwK chains
                lambda f: [c for c, _, _ in walk(f)[2:130]] == list(range(258, 386))))
    out.append(("packbits_flat", W.write(flat, 1, "packbits"), flat, 1, None))  # (a run of row 65 crosses byte 16,384)
    out.append(("lzw_noise_full_table", lzw(noise, fill=True), noise, 1,
                lambda f: (lambda s: s["widths"] == {9, 10, 11, 12} and s["max_entries"] == 4096 and s["after_full"] >= 60
                           and s["clears"] >= 3)(W.lzw(noise.tobytes(), fill=True)[1])))
    out.append(("lzw_clear_lanes", lzw(noise, clear_at=(65, 67, 131)), noise, 1, lambda f: {0, 1, 63} <= _lanes(f, 256)))
    for lane in (0, 1, 63):
        out.append((f"lzw_eoi_lane{lane}", lzw(noise, clear_at=(noise.size - 1 - lane,)), noise, 1,
                    lambda f, lane=lane: _lanes(f, 257) == {lane}))
    a = gray(99, 331)
    out.append(("lzw_no_eoi", lzw(a, eoi=False), a, 1, lambda f: 257 not in [c for c, _, _ in walk(f)]))
    out.append(("lzw_cut", W.write(flat, 1, "lzw", tail=b"\x07" * 300), flat, 1, lambda f: _crosses(f, flat.size)))
    # 256 x 256 tiles of a 300 x 270 image: the edge tiles are clipped
    mask = np.kron(rng.integers(0, 5, (5, 5)), np.ones((64, 64), np.int64))[:270, :300, None].astype(np.uint8)
    out.append(("tiles_palette", T.tiled(mask, 3, "lzw", 256, colormap=T.CMAP), mask, 3, None))
    out.append(("tiles_palette_packbits", T.tiled(mask, 3, "packbits", 256, colormap=T.CMAP), mask, 3, None))
    a = T._px(12, 270, 300, 3)
    out.append(("tiles_rgb_pred2", T.tiled(a, 2, "lzw", 256, pred=2), a, 2, None))
    a = T._px(13, 270, 300, dtype=np.uint16)
    out.append(("tiles_gray16_big", T.tiled(a, 1, "lzw", 256, big=True, pred=2), a, 1, None))
    return out


N_FILES = 17
named = lambda name: next(c for c in files() if c[0] == name)


@functools.lru_cache(None)
def corrupt():
    """Large strips with a sound header: a code above the next free entry, streams that end before their rows."""
    a = TC.image(np.random.default_rng(32), 99, 331, 1, np.uint8)
    f = W.write(a, 1, "lzw")
    at = R.parse(f)[1][273][0] + 20
    return [("code_above_next", f[:at] + b"\xff\xff\xff" + f[at + 3:]),
            ("lzw_truncated", W.write(a, 1, "lzw", codec=lambda d: W.lzw(d[:len(d) // 2])[0])),
            ("packbits_truncated", W.write(a, 1, "packbits", codec=lambda d: W.packbits([d[:-5]])))]
