"""GPU: regions of JPEG files through Context.decode_jpeg_batch(regions=...), bit for bit against the oracle's (CPU)
decode of the whole file, sliced.  A call decodes one file once per region (and whole: None) into the guarded buffer
of tests/jpeg_size_cases.py: padded rows, 0x5A around the records, no byte outside a record's pixels may change."""
import functools
import io
import os

import numpy as np
import pytest

import aeon_amd as A
import oracle
from tests import jpeg_blocks as JB
from tests import jpeg_size_cases as J

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
W, H = 75, 61  # no multiple of any MCU


def _pillow_progressive():
    from PIL import Image
    rng = np.random.default_rng(7)
    a = np.clip(np.add.outer(np.arange(H) * 3, np.arange(W) * 2)[..., None] + rng.integers(0, 90, (H, W, 3)), 0, 255)
    buf = io.BytesIO()
    Image.fromarray(a.astype(np.uint8)).save(buf, "JPEG", quality=85, subsampling=2, progressive=True)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def jpg(name):
    if name in J.YCC:
        return JB.ycc(f"roi_{name}", W, H, J.YCC[name])
    if name in J.FOUR:
        return JB.four(f"roi_{name}", W, H, *J.FOUR[name])
    return {"gray": lambda: JB.gray("roi_gray", W, H),
            "s420_w4": lambda: JB.ycc("roi_s420_w4", 4, H, J.YCC["s420"]),  # chroma 2 samples wide: box replication
            "restart": lambda: JB.ycc("roi_restart", W, H, J.YCC["s420"], restart=3),
            "progressive": _pillow_progressive}[name]()


@functools.lru_cache(maxsize=None)
def want(name, channels):
    a = oracle.jpeg_decode(jpg(name), channels)
    a.setflags(write=False)
    return a


def regions(w, h):
    """Whole (twice); 1x1 at the corners and at odd / odd; inside one block; from odd x, y across one MCU boundary
    each way; up to the last column and row; one sample short of every edge; a full row, a full column."""
    r = [None, (0, 0, w, h), (0, 0, 1, 1), (w - 1, 0, 1, 1), (0, h - 1, 1, 1), (w - 1, h - 1, 1, 1), (1, 1, w - 2, h - 2),
         (0, 31, w, 1), (w // 2, 0, 1, h), (w // 2, 30, w - w // 2, h - 30)]
    if w == W:
        r += [(37, 29, 1, 1), (18, 10, 4, 3), (9, 11, 12, 9), (23, 3, 41, 50)]
    return r


def decode_regions(ctx, files, regs, channels):
    """One guarded call: record i = region regs[i] of files[i] (None: the whole image)."""
    import torch
    sizes = [A.jpeg_info(b)[:2] if r is None else r[2:] for b, r in zip(files, regs)]
    lay, total = J.record_layout(sizes, channels)
    descs = [A.ImgDesc(offset=off, width=w, height=h, stride=stride, channels=channels)
             for (off, stride), (w, h) in zip(lay, sizes)]
    dst = torch.full((total,), J.GUARD, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx.decode_jpeg_batch(files, descs, dst.data_ptr(), stream, regions=regs)
    ctx.synchronize(stream)
    return J.guarded_records(dst.cpu().numpy(), sizes, channels, [str(r) for r in regs])


def check(ctx, name, channels):
    ref = want(name, channels)
    regs = regions(ref.shape[1], ref.shape[0])
    res = decode_regions(ctx, [jpg(name)] * len(regs), regs, channels)
    for r, got in zip(regs, res):
        x, y, w, h = r or (0, 0, ref.shape[1], ref.shape[0])
        bad = np.argwhere(got != ref[y:y + h, x:x + w])
        assert len(bad) == 0, (name, channels, r, len(bad), bad[:3].tolist())
    return res


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = A.Context(0)
    yield c
    c.close()


CASES = [(n, 3) for n in ("s444", "s420", "s422", "s440", "gray", "s420_w4", "cmyk_22", "ycck_420", "progressive",
                          "restart")] + [("s420", 1), ("s422", 1), ("gray", 1), ("cmyk_22", 1), ("progressive", 1)]


@pytest.mark.parametrize("name,channels", CASES)
def test_regions_match_the_whole_decode(ctx, name, channels):
    res = check(ctx, name, channels)
    # the whole image as a region, and as no region, is the plain call
    plain = J.decode_guarded(ctx, [jpg(name)], channels)[0]
    assert np.array_equal(res[0], plain) and np.array_equal(res[1], plain)


@pytest.mark.parametrize("band", [1, 3])
def test_regions_with_short_colour_bands(ctx, band, monkeypatch):
    """AEON_HIP_JPEG_BAND rows per colour workgroup: every band edge inside a region, odd band starts included."""
    monkeypatch.setenv("AEON_HIP_JPEG_BAND", str(band))
    for name in ("s420", "s440", "ycck_420"):
        check(ctx, name, 3)


def test_corrupt_file_among_region_files(ctx):
    """A corrupt entropy-coded file among sound region files: AEON_HIP_EDEVICE from the synchronize, as for whole
    files, and the context decodes the next call correctly."""
    bad = np.load(os.path.join(HERE, "golden", "jpeg_corrupt.npz"))["s411_q85__flip10.jpg"].tobytes()
    with pytest.raises(A.AeonHipError, match="JPEG entropy-coded data corrupt") as e:
        decode_regions(ctx, [jpg("s420"), bad, jpg("s444")], [(9, 11, 12, 9), None, (1, 1, 73, 59)], 3)
    assert e.value.code == A.AEON_HIP_EDEVICE
    check(ctx, "s420", 3)
