"""GPU: the PNG stage (aeon_hip_decode_png_batch: png_inflate and png_unfilter, png_kernels.hip) against the host
decoder and the oracle's PNG decode.  Every file a test lists is asserted to be routed to the device
(aeon_png_host_stage, gpu_route == 1; tests/test_png_stage.py checks the same lists on the CPU): none of the
comparisons below can pass by falling back to the host decoder.  The files come from tests/png_cases.py.
"""
import os
import zlib

import numpy as np
import pytest

import aeon_amd as A
from oracle import png_oracle as PO
from tests import png_cases as PC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FX = np.load(os.path.join(HERE, "golden", "png_fixtures.npz"))
NAMES = sorted({k.rsplit(".", 1)[0] for k in FX.files})
MODES = [(A.PNG_BGR8, "bgr8"), (A.PNG_GRAY8, "gray8"), (A.PNG_ANYDEPTH, "any")]
EDEVICE = -4


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = A.Context(0)
    yield c
    c.close()


def _decode(ctx, files, modes, sync=True):
    """One decode_png_batch call: the records as arrays.  Rows are padded (stride > width) and the buffer is
    pre-filled, so a store outside a row shows."""
    import torch
    descs, shapes, off = [], [], 0
    for b, m in zip(files, modes):
        w, h, d, c = A.png_info(b)
        eb = 2 if (m == A.PNG_ANYDEPTH and d == 16 and c != 3) else 1
        cn = 3 if m == A.PNG_BGR8 else 1
        stride = w * cn * eb + 5 + (len(descs) % 3)
        descs.append(A.ImgDesc(offset=off, width=w, height=h, stride=stride, channels=cn, elem_bytes=eb))
        shapes.append((h, w, cn, eb, stride))
        off += (stride * h + 15) // 16 * 16 + (2 if len(descs) % 2 else 0) * 16
    dst = torch.full((max(off, 16),), 0x5A, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx.decode_png_batch(files, modes, descs, dst.data_ptr(), stream)
    if not sync:
        return None
    ctx.synchronize(stream)
    host = dst.cpu().numpy()
    out = []
    for d, (h, w, cn, eb, stride) in zip(descs, shapes):
        rows = host[d.offset:d.offset + stride * h].reshape(h, stride)
        assert np.all(rows[:, w * cn * eb:] == 0x5A), "bytes written past a row"
        a = np.ascontiguousarray(rows[:, :w * cn * eb])
        a = a.view(np.uint16) if eb == 2 else a
        out.append(a.reshape(h, w, 3) if cn == 3 else a.reshape(h, w))
    return out


def _routed(files):
    for name, png in files:
        for m, _ in MODES:
            assert A.png_host_stage(png, m)[0], (name, "not routed to the device")


def _check_all_modes(ctx, named):
    files = [png for _, png in named for _ in MODES]
    modes = [m for _ in named for m, _ in MODES]
    res = _decode(ctx, files, modes)
    for i, (png, m, r) in enumerate(zip(files, modes, res)):
        want = PO.decode(png, m)
        assert r.dtype == want.dtype and r.shape == want.shape, named[i // 3][0]
        assert np.array_equal(r, want), (named[i // 3][0], m, np.argwhere(r != want)[:3].tolist())


def test_fixtures_one_call_mixed_modes(ctx):
    """Every fixture x three modes in one call, the interlaced ones (host route) among them."""
    inter = [n for n in NAMES if FX[n + ".png"][28] == 1]
    assert inter and len(inter) < len(NAMES)
    for n in NAMES:
        assert A.png_host_stage(FX[n + ".png"].tobytes())[0] == (n not in inter), n
    files = [FX[n + ".png"].tobytes() for n in NAMES for _ in MODES]
    modes = [m for _ in NAMES for m, _ in MODES]
    res = _decode(ctx, files, modes)
    for i, r in enumerate(res):
        n, key = NAMES[i // 3], MODES[i % 3][1]
        want = FX[n + "." + key]
        assert r.dtype == want.dtype and np.array_equal(r, want), (n, key)


def test_inflate_edges_one_batch(ctx):
    cases = PC.inflate_files()
    for name, png, stream, raw in cases:
        assert zlib.decompress(stream) == raw, name
    named = [(name, png) for name, png, _, _ in cases]
    _routed(named)
    _check_all_modes(ctx, named)


def test_filters_on_the_device(ctx):
    named = PC.filter_files() + PC.band_files() + PC.split_files()
    _routed(named)
    _check_all_modes(ctx, named)


@pytest.mark.parametrize("case", range(8))
def test_corrupt_data_is_an_error_not_a_hang(ctx, case):
    name, png = PC.corrupt_files()[case]
    good = PC.filter_files()[3:6]
    _routed([(name, png)] + good)
    import torch
    _decode(ctx, [png], [A.PNG_ANYDEPTH], sync=False)
    with pytest.raises(A.AeonHipError) as e:
        ctx.synchronize(torch.cuda.current_stream().cuda_stream)
    assert e.value.code == EDEVICE and "PNG" in str(e.value), (name, str(e.value))
    _check_all_modes(ctx, good)  # the context is usable, the next batch decodes right


def test_corrupt_cases_are_the_listed_eight():
    assert [n for n, _ in PC.corrupt_files()] == ["adler", "distance", "length_symbol", "oversubscribed", "truncated",
                                                   "too_long", "filter5", "palette_index"]


# ---- the decoder: C5 records (PNG image + PNG mask) whose files the device decodes ------------------------------
IMG64 = dict(height=64, width=64, type="image", channels=3, output_type="float", channel_major=True, bgr_to_rgb=True)
MSK64 = dict(height=64, width=64, type="pixelmask", channels=1, output_type="uint8_t")
VOC = bytes(v for c in range(5) for v in (c * 30, c * 50, 255 - c * 40))


def _c5_window(seed, n=6):
    """n records: an RGB PNG and a palette (8- and 4-bit), gray or 16-bit gray mask of the same size, 64..120 a
    side; with each file's decode by the oracle.  The decoder sends a file through the stage when its stream is at
    most an eighth of its scanlines: the masks (blobs of five classes) and the smooth images of the even records
    go to the device, the noisy images of the odd records stay on the host pool -- both routes in every window."""
    from tests import png_writer as W
    rng = np.random.default_rng(seed)
    recs, decoded = [], []
    for i in range(n):
        w, h = int(rng.integers(64, 121)), int(rng.integers(64, 121))
        img = A.synthetic_image(700 + 10 * seed + i, w, h, 3)
        if i % 2 == 0:  # smooth: ramps, a channel each
            yy, xx = np.mgrid[0:h, 0:w]
            img = np.stack([(xx * 2 + i) % 256, (yy * 3) % 256, (xx + yy) % 256], -1).astype(np.uint8)
        cls = np.kron(rng.integers(0, 5, (8, 8)), np.ones((16, 16), np.int64))[:h, :w].astype(np.uint8)
        ipng = W.write(img[:, :, ::-1], 2, 8, (0, 1, 2, 3, 4) if i % 2 else (4, 1, 2), "fixed" if i % 2 else "dynamic")
        if i % 4 == 0:
            mpng = W.write(cls * 40, 0, 8, (2,))
        elif i % 4 == 1:
            mpng = W.write(cls, 3, 8, (0,), palette=VOC)
        elif i % 4 == 2:
            mpng = W.write(cls.astype(np.uint32) * 9700 + i * 13, 0, 16, (4, 1))
        else:
            mpng = W.write(cls, 3, 4, (0, 2), "fixed", palette=VOC)
        assert A.png_host_stage(ipng, A.PNG_BGR8)[0] and A.png_host_stage(mpng, A.PNG_ANYDEPTH)[0]
        assert A.png_decoder_route(mpng) and A.png_decoder_route(ipng) == (i % 2 == 0), i
        recs.append((ipng, mpng))
        decoded.append((PO.decode(ipng, PO.BGR8), PO.decode(mpng, PO.ANYDEPTH)))
        assert np.array_equal(decoded[-1][0], img)
    return recs, decoded


def _c5_oracle(decoded, params):
    from aeon_amd import configs as C
    from tests import helpers as H
    ref_img = np.stack(H.oracle_records([r[0] for r in decoded], params, C.out_desc_for(IMG64, C.C5_AUG)))
    mod, masks = C.out_desc_for(MSK64, C.C5_AUG), []
    for r, p in zip(decoded, params):
        m = r[1]
        if m.dtype == np.uint16:  # saturate_cast<uchar> of the 16-bit NEAREST result
            lo = H.oracle_records([(m & 0xff).astype(np.uint8)], [p], mod, mask=True)[0]
            hi = H.oracle_records([(m >> 8).astype(np.uint8)], [p], mod, mask=True)[0]
            masks.append(np.minimum(hi.astype(np.uint32) * 256 + lo, 255).astype(np.uint8))
        else:
            masks.append(H.oracle_records([m], [p], mod, mask=True)[0])
    return ref_img, masks


def _c5_cfg(n):
    from aeon_amd import configs as C
    return dict(batch_size=n, random_seed=4, etl=[IMG64, MSK64], augmentation=[C.C5_AUG])


def test_decoder_c5_png_records_decode():
    recs, decoded = _c5_window(1)
    sizes = [(r[0].shape[1], r[0].shape[0]) for r in decoded]
    params = A.Decoder(_c5_cfg(len(recs))).draw_params(sizes)
    img, msk = A.Decoder(_c5_cfg(len(recs))).decode(recs)
    ref_img, ref_msk = _c5_oracle(decoded, params)
    assert np.array_equal(img, ref_img)
    for i, want in enumerate(ref_msk):
        assert np.array_equal(msk[i], want.reshape(msk[i].shape)), i


def test_decoder_c5_png_records_three_windows_submit_wait():
    import torch
    wins = [_c5_window(s) for s in (1, 2, 3)]
    n = len(wins[0][0])
    twin, d = A.Decoder(_c5_cfg(n)), A.Decoder(_c5_cfg(n))
    isz, msz = 3 * 64 * 64 * 4, 64 * 64
    bufs = [(torch.empty(n * isz, dtype=torch.uint8).pin_memory(), torch.empty(n * msz, dtype=torch.uint8).pin_memory())
            for _ in range(2)]
    got = []
    for w in range(2):
        d.submit(wins[w][0], [b.data_ptr() for b in bufs[w]])
    for w in range(3):
        d.wait()
        got.append((bufs[w % 2][0].numpy().view(np.float32).reshape(n, 3, 64, 64).copy(),
                    bufs[w % 2][1].numpy().reshape(n, -1).copy()))
        if w + 2 < 3:
            d.submit(wins[w + 2][0], [b.data_ptr() for b in bufs[w % 2]])
    for w, (recs, decoded) in enumerate(wins):
        params = twin.draw_params([(r[0].shape[1], r[0].shape[0]) for r in decoded])
        ref_img, ref_msk = _c5_oracle(decoded, params)
        assert np.array_equal(got[w][0].reshape(ref_img.shape), ref_img), w
        for i, want in enumerate(ref_msk):
            assert np.array_equal(got[w][1][i], want.reshape(-1)), (w, i)
