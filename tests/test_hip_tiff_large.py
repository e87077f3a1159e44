"""GPU: the files of tests/tiff_large_cases.py through decode_tiff_batch(..., large_strips=True) -- tiff_expand_large over
the strips and tiles above 32 KiB -- into guard-filled strided buffers (tests/test_hip_tiff.py's _decode), against the
pixels each file was cut from, bit for bit."""
import types

import numpy as np
import pytest

import aeon_amd as A
from tests import test_tiff_tiles as T
from tests import tiff_large_cases as LC
from tests import tiff_writer as W
from tests.test_hip_tiff import _decode, ctx  # noqa: F401 (ctx: that module's Context fixture)
from tests.test_tiff_large import routed

pytestmark = pytest.mark.gpu


def Large(ctx):  # the context as _decode calls it, asking for the large strips
    return types.SimpleNamespace(synchronize=ctx.synchronize, decode_tiff_batch=lambda *a: ctx.decode_tiff_batch(*a, large_strips=True))


@pytest.mark.parametrize("k", range(LC.N_FILES))
def test_large_strips_on_the_device(ctx, k):
    name, f, a, photo, _ = LC.files()[k]
    routed(name, f)
    for got, m in zip(_decode(Large(ctx), [f] * 3, T.MODES) + _decode(Large(ctx), [f] * 3, T.MODES), T.MODES * 2):  # (both staging sets)
        T.check(got, a, photo, m, name)


def test_one_call_mixing_large_small_deflate_and_raw(ctx):
    _, both, a, _, _ = LC.named("both_kernels")
    files = [both] +[W.write(a, 1, c, rps=9) for c in ("lzw", "deflate", "raw")]
    routed("both_kernels", files[0])
    assert all(A.tiff_host_stage(f)[0] and A.tiff_large_route(f) for f in files[1:])
    for got in _decode(Large(ctx), files, [A.DECODE_GRAY8] * 4):
        T.check(got, a, 1, A.DECODE_GRAY8, "mixed call")


def test_corrupt_large_strip_among_sound_files(ctx):
    import torch
    (_, good, a, _, _), (_, tiles, mask, _, _) = LC.named("lzw_32769"), LC.named("tiles_palette")
    for name, bad in LC.corrupt():
        files = [good, bad, tiles]
        descs = [A.ImgDesc(offset=(1 << 17) * i, width=p.shape[1], height=p.shape[0], stride=p.shape[1] + 3, channels=1, elem_bytes=1)
                 for i, p in enumerate([a, a, mask])]
        dst, stream = torch.full((3 << 17,), 0x5A, dtype=torch.uint8, device="cuda"), torch.cuda.current_stream().cuda_stream
        ctx.decode_tiff_batch(files, [A.DECODE_GRAY8] * 3, descs, dst.data_ptr(), stream, large_strips=True)
        with pytest.raises(A.AeonHipError) as e:
            ctx.synchronize(stream)
        assert e.value.code == T.EDEVICE and "TIFF" in str(e.value), name
        host = dst.cpu().numpy().reshape(3, 1 << 17)
        for rec, p, photo in ((host[0], a, 1), (host[2], mask, 3)):  # the sound records whole, nothing behind their rows
            h, w = p.shape[:2]
            rows = rec[:h * (w + 3)].reshape(h, w + 3)
            T.check(np.ascontiguousarray(rows[:, :w]), p, photo, A.DECODE_GRAY8, name)
            assert np.all(rows[:, w:] == 0x5A) and np.all(rec[h * (w + 3):] == 0x5A), name
        T.check(_decode(Large(ctx), [good], [A.DECODE_GRAY8])[0], a, 1, A.DECODE_GRAY8, "after " + name)
