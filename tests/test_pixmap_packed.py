"""CPU: the packed pixmap calls (RLE8 / RLE4 and 16-bit BMP files).  The host decoder
(aeon_decode_pixmap_packed) and bmp_rle_expand's code run on the host (aeon_pixmap_gpu_emulate_packed) against the
painted token lists and the numpy shifts of tests/bmp_packed_cases.py, bit for bit; the plain calls still refuse.
"""
import io

import numpy as np
import pytest

import aeon_amd as A
from tests import bmp_packed_cases as C


@pytest.mark.parametrize("decode", [A.decode_pixmap, A.pixmap_gpu_emulate])
def test_good_files_equal_the_reference(decode):
    for name, f, m, want in C.good():
        assert A.pixmap_packed_route(f), name
        assert A.pixmap_info(f, packed=True) == (want.shape[1], want.shape[0], 8, 3, A.PIXMAP_BMP), name
        got = decode(f, m, packed=True)
        assert got.dtype == want.dtype and got.shape == want.shape, (name, m)
        assert np.array_equal(got, want), (name, m, np.argwhere(got != want)[:3].tolist())


@pytest.mark.parametrize("case", C.corrupt(), ids=lambda c: c[0])
def test_corrupt_streams(case):
    name, f = case
    with pytest.raises(A.AeonHipError) as e:
        A.decode_pixmap(f, packed=True)
    assert e.value.code == A.AEON_HIP_EINVAL and "BMP: " in str(e.value) and "RLE data" in str(e.value)
    with pytest.raises(A.AeonHipError) as e:  # the internal -1: what sets the device's corrupt bit
        A.pixmap_gpu_emulate(f, packed=True)
    assert e.value.code == A.AEON_HIP_EDEVICE and "RLE data corrupt" in str(e.value)


def test_rle8_files_equal_pillow():
    from PIL import Image
    for name, f, m, want in C.good():
        if name in C.PILLOW and m == A.DECODE_BGR8:
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))[:, :, ::-1], want), name


def test_the_plain_calls_and_other_variants_stay_refused():
    for name, f, _, _ in C.good()[::3]:
        with pytest.raises(A.AeonHipError) as e:
            A.pixmap_info(f)
        assert e.value.code == A.AEON_HIP_EUNSUPPORTED, name
    w, h, d, toks = C.RLE["width_1"][:4]
    for f, word in ((C.rle_file(w, -h, d, toks), "top-down RLE"), (C.bitfields(C.words(3, 3), 16, (0x0F00, 0xF0, 0xF), False), "masks"),
                    (C.W.bmp(C.words(3, 3), 16, compression=4), "BI_JPEG"), (C.W.bmp(C.words(3, 3), 16, compression=5), "BI_PNG")):
        with pytest.raises(A.AeonHipError, match=word):
            A.pixmap_info(f, packed=True)
