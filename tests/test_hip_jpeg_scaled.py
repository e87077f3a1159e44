"""GPU: JPEG files decoded at 1/2, 1/4 and 1/8 of their size through Context.decode_jpeg_batch(scale=...), bit for
bit against Pillow's libjpeg-turbo at the same scale (draft mode: ISLOW, fancy upsampling), BGR and gray, into the
guarded buffer of tests/jpeg_size_cases.py.  Baseline files take the GPU Huffman decoder (dense coefficients); the
"host" cases take the host entropy decoder's sparse stream: the same images saved progressive, and the files Pillow
cannot write through a context made under AEON_HIP_JPEG_HUFF=host."""
import functools
import io
import os

import numpy as np
import pytest

import aeon_amd as A
from tests import jpeg_blocks as JB
from tests import jpeg_size_cases as J

pytestmark = pytest.mark.gpu
# partial blocks on each edge, odd chroma grids, sizes no multiple of the scale, chroma of one and two samples a row
# (no fancy filter), 153 luma blocks (more than a chunk of any IDCT kernel but the one-lane ones)
SIZES = ((8, 8), (9, 17), (17, 9), (35, 50), (64, 47), (129, 70))
PILLOW = {"gray": None, "s444": 0, "s422": 1, "s420": 2}  # Pillow's subsampling; the others: tests/jpeg_writer.py
LAYOUTS = ("gray", "s444", "s420", "s422", "s440", "s411")
DENSE = dict(nac=8, zmax=64)  # every live coefficient position of the reduced IDCTs


@functools.lru_cache(maxsize=None)
def files(layout, progressive):
    """The layout's files: every size, then two with dense blocks."""
    from PIL import Image
    out = []
    for w, h in SIZES:
        if layout not in PILLOW:
            out.append(JB.ycc(f"sc_{layout}_{w}x{h}", w, h, J.YCC[layout]))
            continue
        rng = np.random.default_rng(w * 1000 + h)
        a = np.add.outer(np.arange(h) * 2, np.arange(w))[..., None] * np.array([1.0, 0.7, 0.4]) + rng.integers(0, 24, (h, w, 3))
        im, buf = Image.fromarray(np.clip(a + 30, 0, 255).astype(np.uint8)), io.BytesIO()
        kw = {} if layout == "gray" else {"subsampling": PILLOW[layout]}
        (im.convert("L") if layout == "gray" else im).save(buf, "JPEG", quality=90, progressive=progressive, **kw)
        out.append(buf.getvalue())
    if layout == "gray":
        out += [JB.gray("sc_dense_gray", 64, 47, draw_kw=DENSE), JB.gray("sc_dense_gray2", 35, 50, draw_kw=DENSE)]
    else:
        samp = J.YCC[layout]
        out += [JB.ycc(f"sc_dense_{layout}", 64, 47, samp, draw_kw=DENSE), JB.ycc(f"sc_dense2_{layout}", 35, 50, samp, draw_kw=DENSE)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pillow(data, s, channels):
    """Pillow's decode of the file at scale s: HWC BGR or HW gray."""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    w, h = im.size
    im.draft("L" if channels == 1 else "RGB", (max(1, w // s), max(1, h // s)))
    assert im.size == (-(-w // s), -(-h // s)), (im.size, w, h, s)  # (the scale asked for is the scale taken)
    a = np.asarray(im)
    if channels == 3:
        a = np.repeat(a[..., None], 3, 2) if a.ndim == 2 else a[..., ::-1]
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def decode_scaled(ctx, data, scales, channels):
    """One guarded call: record i = data[i] at 1 / scales[i]."""
    import torch
    sizes = [(-(-w // s), -(-h // s)) for (w, h, _), s in zip(map(A.jpeg_info, data), scales)]
    lay, total = J.record_layout(sizes, channels)
    descs = [A.ImgDesc(offset=off, width=w, height=h, stride=stride, channels=channels)
             for (off, stride), (w, h) in zip(lay, sizes)]
    dst = torch.full((total,), J.GUARD, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx.decode_jpeg_batch(list(data), descs, dst.data_ptr(), stream, scale=list(scales))
    ctx.synchronize(stream)
    return J.guarded_records(dst.cpu().numpy(), sizes, channels, [f"{A.jpeg_info(b)[:2]} / {s}" for b, s in zip(data, scales)])


@pytest.fixture(scope="module")
def contexts():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    mp = pytest.MonkeyPatch()
    c = {"huff": A.Context(0)}
    mp.setenv("AEON_HIP_JPEG_HUFF", "host")  # (read when the context is created)
    c["host"] = A.Context(0)
    mp.undo()
    yield c
    for x in c.values():
        x.close()


@pytest.mark.parametrize("entropy", ["huff", "host"])
@pytest.mark.parametrize("scale", [2, 4, 8])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_scaled_decode_is_pillows(contexts, layout, scale, entropy):
    ctx, data = contexts[entropy], files(layout, entropy == "host")
    before = ctx.jpeg_launch_counts()
    for channels in (3, 1):
        for b, got in zip(data, decode_scaled(ctx, data, [scale] * len(data), channels)):
            ref = pillow(b, scale, channels)
            assert got.shape == ref.shape, (A.jpeg_info(b), got.shape, ref.shape)
            bad = np.argwhere(got != ref)
            assert len(bad) == 0, (A.jpeg_info(b), channels, len(bad), bad[:3].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])
    after = ctx.jpeg_launch_counts()
    ran = {k for k in after if after[k] > before[k]}
    luma = {2: "idct4", 4: "idct2", 8: "idct1"}[scale]
    chroma = {2: "idct", 4: "idct4", 8: "idct2"}[scale] if layout == "s420" else luma  # (the BGR call's)
    assert ran == {luma, chroma, "color", "scaled"} | ({"huff"} if entropy == "huff" else set()), ran


def test_mixed_scales_in_one_call(contexts):
    """Scales 1, 2, 4 and 8 in one window: every IDCT kernel runs once, and the full-size record is the plain call's."""
    ctx = contexts["huff"]
    data = (files("s420", False)[5], files("gray", False)[3]) * 4
    scales = [1, 1, 2, 2, 4, 4, 8, 8]
    before = ctx.jpeg_launch_counts()
    got = decode_scaled(ctx, data, scales, 3)
    after = ctx.jpeg_launch_counts()
    assert {k: after[k] - before[k] for k in after} == dict(huff=1, idct=1, idct4=1, idct2=1, idct1=1, color=1, color4=0, scaled=1)
    plain = J.decode_guarded(ctx, list(data[:2]), 3)
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    for b, s, g in zip(data[2:], scales[2:], got[2:]):
        assert np.array_equal(g, pillow(b, s, 3)), (A.jpeg_info(b), s)


@pytest.mark.parametrize("scale", [2, 4, 8])
def test_rgb_file_and_a_full_size_cmyk_file(contexts, scale):
    """jpeg_color4's scaled instantiation: an Adobe-RGB file at 1 / scale (Pillow's), next to a CMYK file at scale 1
    (the plain call's record)."""
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cmyk_fixtures.npz"))
    ctx, data = contexts["huff"], (fx["rgb_adobe.jpg"].tobytes(), fx["cmyk_sub2_37x53.jpg"].tobytes())
    for channels in (3, 1):
        before = ctx.jpeg_launch_counts()
        got = decode_scaled(ctx, data, [np.int64(scale), 1], channels)  # (any integer type)
        after = ctx.jpeg_launch_counts()
        assert (after["color4"] - before["color4"], after["color"] - before["color"], after["scaled"] - before["scaled"]) == (1, 0, 1)
        assert np.array_equal(got[0], pillow(data[0], scale, channels))
        assert np.array_equal(got[1], J.decode_guarded(ctx, [data[1]], channels)[0])


@pytest.mark.parametrize("scale", [None, 1, [1, 1]])
def test_unscaled_call_launches_what_it_did(contexts, scale):
    """No scale, or all ones: the whole-size call's kernels, none of the scaled ones."""
    import torch
    ctx, data = contexts["huff"], [files("s420", False)[5], files("gray", False)[3]]
    plain = J.decode_guarded(ctx, data, 3)
    sizes = [A.jpeg_info(b)[:2] for b in data]
    lay, total = J.record_layout(sizes, 3)
    descs = [A.ImgDesc(offset=off, width=w, height=h, stride=stride, channels=3) for (off, stride), (w, h) in zip(lay, sizes)]
    dst = torch.full((total,), J.GUARD, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    before = ctx.jpeg_launch_counts()
    ctx.decode_jpeg_batch(data, descs, dst.data_ptr(), stream, scale=scale)
    ctx.synchronize(stream)
    after = ctx.jpeg_launch_counts()
    assert {k: after[k] - before[k] for k in after} == dict(huff=1, idct=1, idct4=0, idct2=0, idct1=0, color=1, color4=0, scaled=0)
    for a, b in zip(J.guarded_records(dst.cpu().numpy(), sizes, 3), plain):
        assert np.array_equal(a, b)
