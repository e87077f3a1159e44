"""GPU: the files of tests/jpeg_prog_cases.py through decode_jpeg_batch(..., progressive=True) -- jpeg_prog_scan level by
level, jpeg_prog_mask, then the IDCT and colour kernels -- into guard-filled strided buffers
(tests/jpeg_size_cases.decode_guarded), against the oracle's record of each file, bit for bit."""
import functools
import types

import numpy as np
import pytest

import aeon_amd as A
import oracle
from tests import jpeg_prog_cases as PC
from tests import jpeg_size_cases as J
from tests.test_hip_jpeg_sizes import ctx  # noqa: F401 (that module's Context fixture)

pytestmark = pytest.mark.gpu
EDEVICE = -4
NAMES = sorted(PC.files())


def Prog(ctx):  # the context as decode_guarded calls it, asking for the progressive path
    return types.SimpleNamespace(synchronize=ctx.synchronize, decode_jpeg_batch=lambda *a: ctx.decode_jpeg_batch(*a, progressive=True))


@functools.lru_cache(maxsize=None)
def want(f, channels):
    a = oracle.jpeg_decode(f, channels)
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("name", NAMES)
def test_progressive_files_on_the_device(ctx, name, channels):
    f = PC.files()[name]
    assert A.jpeg_prog_route(f), name
    for _ in range(2):  # (both staging sets)
        (got,) = J.decode_guarded(Prog(ctx), [f], channels, [name])
        assert np.array_equal(got, want(f, channels)), (name, channels, int((got != want(f, channels)).sum()))


def test_one_call_mixing_sequential_progressive_gray_and_cmyk(ctx):
    seq = np.load(PC.GOLDEN + "/jpeg_fixtures.npz")["s420_q50.jpg"].tobytes()
    files = [seq] + [PC.files()[k] for k in ("s420_17x9_q95", "gray_33x70_q75", "prog_cmyk")]
    assert [A.jpeg_prog_route(f) for f in files] == [False, True, True, True]
    for cn in (3, 1):
        for f, got in zip(files, J.decode_guarded(Prog(ctx), files, cn)):
            assert np.array_equal(got, want(f, cn)), cn


def test_corrupt_scan_among_sound_files(ctx):
    import torch
    good, bad, gray = PC.files()["s420_17x9_q95"], PC.corrupt(), PC.files()["gray_33x70_q75"]
    files, sizes = [good, bad, gray], [A.jpeg_info(f)[:2] for f in (good, bad, gray)]
    lay, total = J.record_layout(sizes, 3)
    descs = [A.ImgDesc(offset=off, width=w, height=h, stride=stride, channels=3) for (off, stride), (w, h) in zip(lay, sizes)]
    dst, stream = torch.full((total,), J.GUARD, dtype=torch.uint8, device="cuda"), torch.cuda.current_stream().cuda_stream
    with pytest.raises(A.AeonHipError):  # without the flag the host decoder refuses the file at the call
        ctx.decode_jpeg_batch(files, descs, dst.data_ptr(), stream)
    ctx.synchronize(stream)
    ctx.decode_jpeg_batch(files, descs, dst.data_ptr(), stream, progressive=True)  # the call itself returns
    with pytest.raises(A.AeonHipError) as e:
        ctx.synchronize(stream)
    assert e.value.code == EDEVICE and "JPEG" in str(e.value)
    sound = J.guarded_records(dst.cpu().numpy(), sizes, 3)  # the sound records whole, every guard byte untouched
    assert np.array_equal(sound[0], want(good, 3)) and np.array_equal(sound[2], want(gray, 3))
    (again,) = J.decode_guarded(Prog(ctx), [good], 3)
    assert np.array_equal(again, want(good, 3))


def test_regions_of_progressive_files_stay_on_the_host(ctx):
    f = PC.files()["s444_8x8_q90"]
    with pytest.raises(ValueError):
        ctx.decode_jpeg_batch([f], [A.ImgDesc(offset=0, width=4, height=4, stride=12, channels=3)], 0, 0, regions=[(0, 0, 4, 4)], progressive=True)
