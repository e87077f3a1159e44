"""GPU: the files of tests/test_tiff_tiles.py through the TIFF stage (tiff_expand over the tiles, tiff_convert_tiled over
the tiled bands) against the pixels they were cut from; then the Decoder and the stager's encoded records."""
import numpy as np
import pytest

import aeon_amd as A
from aeon_amd import configs as C
from tests import helpers as H
from tests import test_hip_stager_encoded as E
from tests import test_tiff_tiles as T
from tests import tiff_writer as W
from tests.test_hip_tiff import IMG64, _decode, ctx  # noqa: F401 (ctx: that module's Context fixture)

pytestmark = pytest.mark.gpu
BGR8, GRAY8 = A.DECODE_BGR8, A.DECODE_GRAY8


@pytest.mark.parametrize("geometry,comp", T.CASES)
def test_geometry_on_the_device(ctx, geometry, comp):
    a, photo, f, device = T.case_file(geometry, comp)
    assert A.tiff_host_stage(f)[0] is device  # (the 64 KiB LZW / PackBits tiles: the call's host route)
    for got, m in zip(_decode(ctx, [f] * 3, T.MODES) + _decode(ctx, [f] * 3, T.MODES), T.MODES * 2):  # (both staging sets)
        T.check(got, a, photo, m, geometry)


def test_tiled_strip_and_truncated_files_in_one_call(ctx):  # both convert kernels; the sound records stay whole
    import torch
    a = T._px(11, 48, 48, 3)
    files = [T.tiled(a, 2, "lzw", pred=2), W.write(a, 2, "lzw", pred=2, rps=5), T.tiled(a, 2, "lzw", tags=T.TRUNCATED)]
    assert all(A.tiff_host_stage(f) == (True, len(f)) for f in files)
    descs = [A.ImgDesc(offset=8192 * i, width=48, height=48, stride=144, channels=3, elem_bytes=1) for i in range(3)]
    dst, stream = torch.zeros(3 * 8192, dtype=torch.uint8, device="cuda"), torch.cuda.current_stream().cuda_stream
    ctx.decode_tiff_batch(files, [BGR8] * 3, descs, dst.data_ptr(), stream)
    with pytest.raises(A.AeonHipError) as e:
        ctx.synchronize(stream)
    assert e.value.code == T.EDEVICE and "TIFF" in str(e.value)
    for rec in dst.cpu().numpy().reshape(3, 8192)[:2]:
        T.check(rec[:48 * 144].reshape(48, 48, 3), a, 2, BGR8, "beside a truncated tile")
    T.check(_decode(ctx, files[:1], [GRAY8])[0], a, 2, GRAY8, "after a truncated tile")


def test_decoder_and_stager_take_tiled_records(ctx):
    imgs = [A.synthetic_image(900 + i, 70 + 10 * i, 120 - 9 * i, 3) for i in range(E.BATCH)]
    files = [T.tiled(im[:, :, ::-1], 2, ["lzw", "raw"][i % 2], 32, pred=2 - i % 2, reverse=i > 1) for i, im in enumerate(imgs)]
    assert all(A.tiff_decoder_route(f) for f in files)
    sizes = [(a.shape[1], a.shape[0]) for a in imgs]
    cfg = dict(batch_size=len(files), random_seed=9, etl=[IMG64], augmentation=[C.C5_AUG])
    want = H.oracle_records(imgs, A.Decoder(cfg).draw_params(sizes), C.out_desc_for(IMG64, C.C5_AUG))
    assert np.array_equal(A.Decoder(cfg).decode([(f,) for f in files])[0], np.stack(want))
    params, out = H.draw_params(C.C2_AUG, sizes, E.OUT_W, E.OUT_H, seed=E.SEED), E._out()
    st, buf = A.Stager(ctx, out, E.BATCH), E.Guarded(E.BATCH * out.item_stride, "pinned")
    E._stage_window(st, [buf], files, params)
    st.flush(buf.ptr)
    E._assert_items(buf.items(E.BATCH, out.item_stride, E.ITEM), E._reference(imgs, params, out), "tiled")
    assert st.last_decode()["device"]["tiff"] == E.BATCH
    st.close(), buf.free()
