"""Tiled TIFF files on the CPU: Pillow, the host decoder and the stage's kernel code run on the host
(tiff_gpu_emulate) against the pixels each file was cut from; then the refusals and the table checks."""
import io
import struct
import zlib

import numpy as np
import pytest

import aeon_amd as A
from tests import tiff_ref as R
from tests import tiff_writer as W

MODES, (EINVAL, EUNSUPPORTED, EDEVICE) = [A.DECODE_BGR8, A.DECODE_GRAY8, A.DECODE_ANYDEPTH], (-1, -3, -4)


def tiled(a, photo, comp="raw", tile=16, big=False, pred=1, colormap=None, reverse=False, tags={}):
    """The file: header, square tiles (cut from `a`, HxWxS, padded with 0xA5; reverse: stored last tile first, each
    behind one stray byte, so at odd offsets too), tag values, IFD.  tags: {tag: (type, values) or None} over the IFD's."""
    (h, w, spp), bps, E = a.shape, 8 * a.itemsize, ">" if big else "<"
    full = np.full((-(-h // tile) * tile, -(-w // tile) * tile, spp), 0xA5, a.dtype)
    full[:h, :w] = a
    body, at = bytearray(8), []
    tiles = [full[y:y + tile, x:x + tile] for y in range(0, len(full), tile) for x in range(0, full.shape[1], tile)]
    for t in tiles[::-1] if reverse else tiles:
        if pred == 2:
            t = np.concatenate([t[:, :1], t[:, 1:] - t[:, :-1]], axis=1)  # (wraps mod 2^bps)
        rows = [r.astype(E + "u2" if bps == 16 else np.uint8).tobytes() for r in t]
        blob = {"raw": b"".join, "lzw": lambda r: W.lzw(b"".join(r))[0], "packbits": W.packbits,
                "deflate": lambda r: zlib.compress(b"".join(r))}[comp](rows)
        at.append((len(body) + reverse, len(blob)))
        body += b"\x77" * reverse + blob
    at = at[::-1] if reverse else at
    T = {256: (4, [w]), 257: (4, [h]), 258: (3, [bps] * spp), 259: (3, [W.COMP[comp]]), 262: (3, [photo]), 277: (3, [spp]),
         317: (3, [pred]), 322: (3, [tile]), 323: (3, [tile]), 324: (4, [o for o, _ in at]), 325: (4, [n for _, n in at]),
         338: (3, [1]) if spp in (2, 4) else None,  # one associated extra sample
         320: (3, [int(v) for v in colormap.T.reshape(-1)]) if photo == 3 else None, **tags}
    ifd = b""
    for t, (ty, v) in sorted((t, v) for t, v in T.items() if v):
        data = struct.pack(E + {3: "H", 4: "I"}[ty] * len(v), *v)
        ifd += struct.pack(E + "HHI", t, ty, len(v)) + (data.ljust(4, b"\0") if len(data) <= 4 else struct.pack(E + "I", len(body)))
        body += data if len(data) > 4 else b""
    body[:8] = (b"MM" if big else b"II") + struct.pack(E + "HI", 42, len(body))
    return bytes(body + struct.pack(E + "H", len(ifd) // 12) + ifd + bytes(4))


def check(got, a, photo, mode, what):  # `got` against tests/tiff_ref.py's conversions of the source pixels `a`
    if photo == 1:
        v = a[:, :, 0] if a.itemsize == 1 or mode == A.DECODE_ANYDEPTH else (a[:, :, 0] >> 8).astype(np.uint8)
        want = np.dstack([v, v, v]) if mode == A.DECODE_BGR8 else v
    else:
        c = a[:, :, :3] if photo == 2 else (CMAP >> 8).astype(np.uint8)[a[:, :, 0]]  # HxWx3 RGB
        want = c[:, :, ::-1] if mode == A.DECODE_BGR8 else R.gray_of(c[:, :, 2], c[:, :, 1], c[:, :, 0])
    assert got.dtype == want.dtype and np.array_equal(got, want), (what, mode, np.argwhere(got != want)[:3].tolist())


def _px(seed, h, w, spp=1, dtype=np.uint8):  # ramps with some noise: every codec gets runs and literals
    ramp, top = np.add.outer(np.arange(h) * 3, np.arange(w) * 5)[:, :, None], 256 ** np.dtype(dtype).itemsize
    return ((ramp * (top // 256) + np.random.default_rng(seed).integers(0, 4, (h, w, spp)) * (top // 64)) % top).astype(dtype)


CMAP = (np.arange(768).reshape(256, 3) * 157 % 65536).astype(np.uint16)
GEOMETRY = {  # name: (pixels, photo, keywords of tiled())
    "40x35 rgb, edge tiles": (_px(1, 35, 40, 3), 2, {}),
    "5x3 in one tile": (_px(2, 3, 5), 1, {}),
    "32x16, no padding": (_px(3, 16, 32), 1, {}),
    "rgb predictor 2": (_px(4, 35, 40, 3), 2, dict(pred=2)),
    "gray16 big-endian predictor 2": (_px(5, 35, 40, dtype=np.uint16), 1, dict(pred=2, big=True)),
    "palette": (_px(6, 35, 40), 3, dict(colormap=CMAP)),
    "rgb + associated extra": (_px(7, 35, 40, 4) | np.array([0, 0, 0, 255], np.uint8), 2, {}),  # (Pillow divides by alpha)
    "reverse order, odd offsets": (_px(8, 35, 40, 3), 2, dict(reverse=True)),
    "6000x16 rgb": (_px(9, 16, 6000, 3), 2, {}),
    "256x256 tiles": (_px(10, 300, 260), 1, dict(tile=256)),  # (64 KiB: LZW / PackBits tiles above the device's cap)
}
CASES = [(g, c) for g in GEOMETRY for c in ("raw", "lzw", "deflate", "packbits")]
TRUNCATED = {325: (4, [40] * 9)}  # a sound header over tiles cut to 40 bytes: only the tile's decoder can tell


def case_file(geometry, comp):  # -> pixels, photo, the file, does the device take it
    a, photo, kw = GEOMETRY[geometry]
    f = tiled(a, photo, comp, **(dict(kw, pred=1) if comp in ("raw", "packbits") else kw))  # (no predictor under those)
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(f))).reshape(a.shape), a), "Pillow reads other pixels"
    return a, photo, f, not (kw.get("tile") == 256 and comp in ("lzw", "packbits"))


@pytest.mark.parametrize("geometry,comp", CASES)
def test_host_decode_and_emulation_give_the_source_pixels(geometry, comp):
    a, photo, f, device = case_file(geometry, comp)
    assert A.tiff_info(f) == (a.shape[1], a.shape[0], 3 if photo >= 2 else 1, a.itemsize)
    for m in MODES:
        assert A.tiff_host_stage(f, m)[0] is device and (A.tiff_decoder_route(f) is device or comp == "deflate")
        check(A.decode_tiff(f, m), a, photo, m, "host")
        if device:
            check(A.tiff_gpu_emulate(f, m), a, photo, m, "emulation")


@pytest.mark.parametrize("tags,code,named", [
    ({323: None, 324: None, 325: None}, EUNSUPPORTED, "TileWidth"), ({322: (3, [24])}, EUNSUPPORTED, "TileWidth"),
    ({323: (3, [8])}, EUNSUPPORTED, "TileLength"), ({324: (4, [8] * 8)}, EINVAL, "9"), ({325: (4, [4] * 10)}, EINVAL, "9"),
    ({324: (4, [8] * 8 + [1 << 20])}, EINVAL, "tile 8"), ({325: (4, [4] * 8 + [1 << 20])}, EINVAL, "tile 8"),
    (TRUNCATED, EINVAL, "tile 0")])
def test_refusals_table_checks_and_a_truncated_tile(tags, code, named):
    f = tiled(_px(1, 35, 40), 1, "lzw", tags=tags)
    with pytest.raises(A.AeonHipError) as e:
        A.decode_tiff(f)
    msg = str(e.value).split(": ", 1)[1]
    assert e.value.code == code and msg.startswith("TIFF: ") and named in msg, msg
    assert msg.endswith("not supported") is (code == EUNSUPPORTED), msg
    with pytest.raises(A.AeonHipError) as e:  # the header's refusals before any decode; a truncated tile on the "device"
        (A.tiff_gpu_emulate if tags is TRUNCATED else A.tiff_info)(f)
    assert e.value.code == (EDEVICE if tags is TRUNCATED else code) and (tags is TRUNCATED or str(e.value).endswith(msg))
