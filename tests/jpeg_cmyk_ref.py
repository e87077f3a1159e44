"""The yardstick of the CMYK / YCCK / Adobe-RGB JPEG decode: what cv::imdecode (OpenCV 2.4, aeon's
image::extractor::extract, src/etl_image.cpp:83-99) makes of libjpeg's output for such files, restated
on numpy integers.

The input is libjpeg's raw samples after upsampling: for a 4-component file the C, M, Y, K planes as
jdcolor.c hands them over (a YCCK file after ycck_cmyk_convert), for an RGB file its R, G, B planes.
Pillow decodes to exactly those planes and then inverts every CMYK JPEG, so raw = 255 - Pillow's
decode (raw_from_pillow).  From there:

  ycck_to_cmyk   jdcolor.c ycck_cmyk_convert (16-bit fixed-point tables, K copied)
  cmyk_to_bgr    OpenCV 2.4 icvCvt_CMYK2BGR_8u_C4C3R:  c = k - ((255 - c) * k >> 8), B, G, R = y, m, c
  cmyk_to_gray   icvCvt_CMYK2Gray_8u_C4C1R:            (y * 1868 + m * 9617 + c * 4899 + 8192) >> 14
  rgb_to_bgr     the planes swapped
  rgb_to_gray    libjpeg-turbo rgb_gray_convert:        (R * 19595 + G * 38470 + B * 7471 + 32768) >> 16

The entropy decode, IDCT, upsampling and the YCCK conversion are pinned by Pillow / libjpeg-turbo; the
three OpenCV formulas and the RGB -> gray formula are restated from their sources and not pinned by a
run of OpenCV.  All arithmetic is int32; every result fits uint8 without a clamp except where one is
written.
"""
import numpy as np


def raw_from_pillow(decoded):
    """libjpeg's samples from Pillow's decode: Pillow inverts every CMYK JPEG (with or without an
    Adobe marker); an RGB decode is returned as it is."""
    a = np.asarray(decoded)
    return 255 - a if a.ndim == 3 and a.shape[2] == 4 else a


def ycck_to_cmyk(ycck):
    """jdcolor.c ycck_cmyk_convert on HxWx4 (Y, Cb, Cr, K) samples."""
    a = np.asarray(ycck).astype(np.int32)
    y, cb, cr, k = a[..., 0], a[..., 1] - 128, a[..., 2] - 128, a[..., 3]
    cr_r = (91881 * cr + 32768) >> 16
    cb_b = (116130 * cb + 32768) >> 16
    g = (-22554 * cb + (-46802 * cr + 32768)) >> 16
    c = np.clip(255 - (y + cr_r), 0, 255)
    m = np.clip(255 - (y + g), 0, 255)
    ye = np.clip(255 - (y + cb_b), 0, 255)
    return np.stack([c, m, ye, k], axis=-1).astype(np.uint8)


def _cmy_over_k(cmyk):
    a = np.asarray(cmyk).astype(np.int32)
    k = a[..., 3]
    return [k - (((255 - a[..., i]) * k) >> 8) for i in range(3)]


def cmyk_to_bgr(cmyk):
    """icvCvt_CMYK2BGR_8u_C4C3R on libjpeg's raw HxWx4 samples."""
    c, m, y = _cmy_over_k(cmyk)
    return np.stack([y, m, c], axis=-1).astype(np.uint8)


def cmyk_to_gray(cmyk):
    """icvCvt_CMYK2Gray_8u_C4C1R on libjpeg's raw HxWx4 samples."""
    c, m, y = _cmy_over_k(cmyk)
    return ((y * 1868 + m * 9617 + c * 4899 + 8192) >> 14).astype(np.uint8)


def rgb_to_bgr(rgb):
    return np.ascontiguousarray(np.asarray(rgb)[..., ::-1])


def rgb_to_gray(rgb):
    """libjpeg-turbo's rgb_gray_convert (JCS_RGB source, JCS_GRAYSCALE output)."""
    a = np.asarray(rgb).astype(np.int32)
    return ((a[..., 0] * 19595 + a[..., 1] * 38470 + a[..., 2] * 7471 + 32768) >> 16).astype(np.uint8)


def decode(raw):
    """(BGR, gray) of a file from its raw samples: HxWx4 CMYK (a YCCK file already converted) or
    HxWx3 RGB."""
    raw = np.asarray(raw)
    if raw.shape[2] == 4:
        return cmyk_to_bgr(raw), cmyk_to_gray(raw)
    return rgb_to_bgr(raw), rgb_to_gray(raw)
