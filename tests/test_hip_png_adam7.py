"""GPU: Adam7-interlaced PNG files through the opt-in call (aeon_hip_decode_png_interlaced_batch: png_inflate, then
png_unfilter_adam7, one wave per file and pass) against the oracle, bit for bit.  Every file is asserted routed by
aeon_png_interlaced_route, so none of the comparisons can pass by the host decoder.  The files are
tests/test_png_adam7.py's lists.
"""
import numpy as np
import pytest

import aeon_amd as A
from oracle import png_oracle as PO
from tests import test_png_adam7 as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = A.Context(0)
    yield c
    c.close()


def _decode(ctx, files, modes, interlaced=True, sync=True):
    """One decode_png_batch call into padded, pre-filled records at odd offsets: the records as arrays."""
    import torch
    descs, shapes, off = [], [], 1
    for b, m in zip(files, modes):
        w, h, d, c = A.png_info(b)
        eb = 2 if (m == A.PNG_ANYDEPTH and d == 16 and c != 3) else 1
        cn = 3 if m == A.PNG_BGR8 else 1
        stride = w * cn * eb + 5 + (len(descs) % 3)
        descs.append(A.ImgDesc(offset=off, width=w, height=h, stride=stride, channels=cn, elem_bytes=eb))
        shapes.append((h, w, cn, eb, stride))
        off += stride * h + 7 + 2 * (len(descs) % 4)
    dst = torch.full((off + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx.decode_png_batch(files, modes, descs, dst.data_ptr(), stream, interlaced=interlaced)
    if not sync:
        return None
    ctx.synchronize(stream)
    host, out, end = dst.cpu().numpy(), [], 0
    for d, (h, w, cn, eb, stride) in zip(descs, shapes):
        assert np.all(host[end:d.offset] == 0x5A), "bytes written between records"
        rows = host[d.offset:d.offset + stride * h].reshape(h, stride)
        assert np.all(rows[:, w * cn * eb:] == 0x5A), "bytes written past a row"
        a = np.ascontiguousarray(rows[:, :w * cn * eb])
        a = a.view(np.uint16) if eb == 2 else a
        out.append(a.reshape(h, w, 3) if cn == 3 else a.reshape(h, w))
        end = d.offset + stride * h
    return out


def _check_all_modes(ctx, named, interlaced=True):
    files = [png for _, png in named for _ in L.MODES]
    modes = [m for _ in named for m, _ in L.MODES]
    for name, png in named:
        assert A.png_interlaced_route(png) or not interlaced, (name, "not routed to the device")
    for i, r in enumerate(_decode(ctx, files, modes, interlaced)):
        want = PO.decode(files[i], modes[i])
        assert r.dtype == want.dtype and r.shape == want.shape, named[i // 3][0]
        assert np.array_equal(r, want), (named[i // 3][0], modes[i], np.argwhere(r != want)[:3].tolist())


def _fixtures():
    """The interlaced fixtures and their plain twins, mixed in one call."""
    return [(n, L.FX[n + ".png"].tobytes()) for i in L.INTER for n in (i, i[:-2] + "_n")]


@pytest.mark.parametrize("files", [_fixtures, L.size_files, L.depth_files, L.band_files])
def test_one_call(ctx, files):
    _check_all_modes(ctx, files())


@pytest.mark.parametrize("case", range(3))
def test_corrupt_data_in_a_pass_is_an_error(ctx, case):
    import torch
    name, png = L.corrupt_files()[case]
    assert A.png_interlaced_route(png), name
    _decode(ctx, [png], [A.PNG_ANYDEPTH], sync=False)
    with pytest.raises(A.AeonHipError) as e:
        ctx.synchronize(torch.cuda.current_stream().cuda_stream)
    assert e.value.code == L.EDEVICE and "PNG" in str(e.value), (name, str(e.value))
    _check_all_modes(ctx, _fixtures()[:6])  # the context is usable, the next batch decodes right


def test_plain_call_keeps_interlaced_files_on_the_host(ctx):
    named = [(n, L.FX[n + ".png"].tobytes()) for n in ("pal4_i", "c6_16_i")]
    assert not any(A.png_host_stage(png)[0] for _, png in named)
    _check_all_modes(ctx, named, interlaced=False)
