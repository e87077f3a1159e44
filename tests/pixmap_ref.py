"""A numpy restatement of the pixmap decode rules, written from the rules and not from the
product: the yardstick aeon_decode_pixmap, the emulation and the kernel are compared with.  decode(data, mode)
returns HxWx3 uint8 (BGR8), HxW uint8 (GRAY8) or HxW uint8 / uint16 (ANYDEPTH); Refused carries the code
(-1 invalid, -3 unsupported) and whether the message must start with "BMP:" or "PNM:".
"""
import struct

import numpy as np

BGR8, GRAY8, ANYDEPTH = 0, 1, 2
EINVAL, EUNSUPPORTED = -1, -3
WS = b" \t\n\v\f\r"


class Refused(Exception):
    def __init__(self, code, prefix, why):
        super().__init__(f"{prefix} {why}")
        self.code, self.prefix = code, prefix


def gray(b, g, r):
    """(B*1868 + G*9617 + R*4899 + 8192) >> 14, on 8- or 16-bit samples."""
    return (b.astype(np.uint64) * 1868 + g.astype(np.uint64) * 9617 + r.astype(np.uint64) * 4899 + 8192) >> 14


def _finish(bgr, mode, wide):
    """bgr: HxWx3 samples (uint16 when wide) or HxW gray samples -> the record of `mode`."""
    is_gray = bgr.ndim == 2
    if wide and mode != ANYDEPTH:
        bgr = bgr >> 8  # each sample becomes v >> 8
    if mode == BGR8:
        return (np.repeat(bgr[:, :, None], 3, 2) if is_gray else bgr).astype(np.uint8)
    g = bgr if is_gray else gray(bgr[:, :, 0], bgr[:, :, 1], bgr[:, :, 2])
    return g.astype(np.uint16 if (wide and mode == ANYDEPTH) else np.uint8)


class _Tokens:
    def __init__(self, d, p):
        self.d, self.p = d, p

    def skip(self):
        d = self.d
        while self.p < len(d):
            if d[self.p] in WS:
                self.p += 1
            elif d[self.p] == ord("#"):
                while self.p < len(d) and d[self.p] not in b"\n\r":
                    self.p += 1
            else:
                break

    def number(self):
        self.skip()
        d, q = self.d, self.p
        while q < len(d) and 48 <= d[q] <= 57:
            q += 1
        if q == self.p:
            raise Refused(EINVAL, "PNM:", "a number is missing")
        v = int(d[self.p:q])
        if v > 2 ** 31 - 1:
            raise Refused(EINVAL, "PNM:", "number too large")
        self.p = q
        return v

    def bit(self):
        self.skip()
        if self.p >= len(self.d) or self.d[self.p] not in b"01":
            raise Refused(EINVAL, "PNM:", "a bit is missing")
        self.p += 1
        return self.d[self.p - 1] - 48


def _pnm(d, mode):
    magic = d[1] - 48
    t = _Tokens(d, 2)
    w, h = t.number(), t.number()
    maxval = 1 if magic in (1, 4) else t.number()
    if not 1 <= maxval <= 65535 or w < 1 or h < 1 or w * h > 2 ** 28:
        raise Refused(EINVAL, "PNM:", "limits")
    if t.p >= len(d) or d[t.p] not in WS:
        raise Refused(EINVAL, "PNM:", "one whitespace byte follows the last token")
    p = t.p + 1
    cn = 3 if magic in (3, 6) else 1
    wide = maxval > 255
    if magic == 4:
        rowb = (w + 7) // 8
        if len(d) - p < rowb * h:
            raise Refused(EINVAL, "PNM:", "short")
        bits = np.unpackbits(np.frombuffer(d, np.uint8, rowb * h, p).reshape(h, rowb), axis=1)[:, :w]
        s = np.where(bits == 0, 255, 0)
    elif magic in (5, 6):
        n = w * h * cn
        if len(d) - p < n * (2 if wide else 1):
            raise Refused(EINVAL, "PNM:", "short")
        s = np.frombuffer(d, ">u2" if wide else np.uint8, n, p).astype(np.uint16)  # as they are: no scaling
    else:
        t.p = p
        n = w * h * cn
        try:
            if magic == 1:
                s = np.array([255 if t.bit() == 0 else 0 for _ in range(n)])
            else:
                v = np.minimum(np.array([t.number() for _ in range(n)], np.int64), maxval)
                s = v if wide else v * 255 // maxval
        except Refused:
            raise Refused(EINVAL, "PNM:", "the ASCII data runs out of samples")
    s = np.asarray(s).astype(np.uint16)
    if cn == 3:
        return _finish(s.reshape(h, w, 3)[:, :, ::-1], mode, wide)
    return _finish(s.reshape(h, w), mode, wide)


def _bmp(d, mode):
    if len(d) < 18:
        raise Refused(EINVAL, "BMP:", "short")
    off, hs = struct.unpack_from("<I", d, 10)[0], struct.unpack_from("<I", d, 14)[0]
    if hs != 12 and hs < 40:
        raise Refused(EINVAL, "BMP:", "info header size")
    if 14 + hs > len(d):
        raise Refused(EINVAL, "BMP:", "short header")
    comp, used = 0, 0
    if hs == 12:
        w, h, _, bpp = struct.unpack_from("<HHHH", d, 18)
    else:
        w, h, _, bpp, comp = struct.unpack_from("<iiHHI", d, 18)
        used = struct.unpack_from("<I", d, 46)[0]
    if w < 1 or h == 0 or w * abs(h) > 2 ** 28:
        raise Refused(EINVAL, "BMP:", "size")
    if comp in (1, 2):
        raise Refused(EUNSUPPORTED, "BMP:", "RLE")
    if comp == 3 or bpp == 16:
        raise Refused(EUNSUPPORTED, "BMP:", "16-bit")
    if comp != 0 or bpp not in (1, 4, 8, 24, 32):
        raise Refused(EINVAL, "BMP:", "variant")
    pal = np.zeros((256, 3), np.uint8)
    if bpp <= 8:
        n = (1 << bpp) if (hs == 12 or used == 0) else used
        esz = 3 if hs == 12 else 4
        if n > 256:
            raise Refused(EINVAL, "BMP:", "palette too long")
        if 14 + hs + n * esz > len(d):
            raise Refused(EINVAL, "BMP:", "short palette")
        pal[:n] = np.frombuffer(d, np.uint8, n * esz, 14 + hs).reshape(n, esz)[:, :3]
    ah = abs(h)
    pitch = ((w * bpp + 7) // 8 + 3) & ~3
    if off + pitch * ah > len(d):
        raise Refused(EINVAL, "BMP:", "short pixel data")
    rows = np.frombuffer(d, np.uint8, pitch * ah, off).reshape(ah, pitch)
    if h > 0:
        rows = rows[::-1]
    if bpp <= 8:
        if bpp == 1:
            idx = np.unpackbits(rows, axis=1)[:, :w]
        elif bpp == 4:
            idx = np.stack([rows >> 4, rows & 15], 2).reshape(ah, -1)[:, :w]
        else:
            idx = rows[:, :w]
        if mode == BGR8:
            return pal[idx]
        pg = gray(pal[:, 0], pal[:, 1], pal[:, 2]).astype(np.uint8)  # the gray of the palette entry
        return pg[idx]
    spp = bpp // 8
    px = rows[:, :w * spp].reshape(ah, w, spp)[:, :, :3]  # 32-bit: the fourth byte is dropped
    return _finish(px.astype(np.uint16), mode, False)


def decode(data, mode):
    d = bytes(data)
    if len(d) >= 3 and d[0] == ord("P") and ord("1") <= d[1] <= ord("6") and d[2] in WS:
        return _pnm(d, mode)
    if d[:2] == b"BM":
        return _bmp(d, mode)
    raise Refused(EINVAL, "", "neither")
