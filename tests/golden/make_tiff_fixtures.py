"""Writes tests/golden/tiff_fixtures.npz: TIFF files written by Pillow (libtiff) -- modes L, RGB, RGBA, P and I;16
under compression raw, tiff_lzw, tiff_adobe_deflate, tiff_deflate and packbits, with Predictor and RowsPerStrip
passed through tiffinfo where libtiff takes them -- each stored with Pillow's decode of it: NAME.file the bytes,
NAME.pil the pixels Pillow reads back (RGB order; P files converted to RGB), NAME.mode Pillow's mode.

    python tests/golden/make_tiff_fixtures.py
"""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def picture(rng, h, w, cn, top=256):
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([(x * (5 + 2 * c) * (top // 256) + y * 3 * (top // 256) + 37 * c) % top for c in range(cn)], axis=2)
    a = a + rng.integers(0, 6, a.shape) * (top // 256)
    a[h // 3:h // 3 + 3] = a[h // 3]
    return a % top


def main():
    rng = np.random.default_rng(7)
    out = {}
    k = 0
    for comp in ["raw", "tiff_lzw", "tiff_adobe_deflate", "tiff_deflate", "packbits"]:
        for mode in ["L", "RGB", "RGBA", "P", "I;16"]:
            for variant in range(2):
                w, h = [(37, 29), (64, 48), (130, 21), (9, 70)][k % 4]
                k += 1
                if mode == "I;16":
                    im = Image.fromarray(picture(rng, h, w, 1, 65536)[:, :, 0].astype(np.uint16))
                elif mode == "P":
                    im = Image.fromarray((picture(rng, h, w, 1)[:, :, 0] % 40).astype(np.uint8), "P")
                    im.putpalette([int(v) for v in rng.integers(0, 256, 768)])
                else:
                    cn = dict(L=1, RGB=3, RGBA=4)[mode]
                    a = picture(rng, h, w, cn).astype(np.uint8)
                    im = Image.fromarray(a[:, :, 0] if cn == 1 else a, mode)
                info = {}
                if variant:
                    info[278] = [1, 5, 16, h][k % 4]  # RowsPerStrip
                    if comp in ("tiff_lzw", "tiff_adobe_deflate", "tiff_deflate") and mode != "P":
                        info[317] = 2  # Predictor
                buf = io.BytesIO()
                im.save(buf, "TIFF", compression=None if comp == "raw" else comp, tiffinfo=info)
                f = buf.getvalue()
                back = Image.open(io.BytesIO(f))
                back.load()
                px = np.array(back.convert("RGB") if back.mode == "P" else back)
                name = f"{comp}_{mode.replace(';', '')}_{variant}"
                out[name + ".file"] = np.frombuffer(f, np.uint8)
                out[name + ".pil"] = px
                out[name + ".mode"] = np.array(back.mode)
    np.savez_compressed(os.path.join(HERE, "tiff_fixtures.npz"), **out)
    print(len(out) // 3, "files,", sum(v.nbytes for v in out.values()), "bytes")


if __name__ == "__main__":
    main()
