"""GPU: the TIFF stage (aeon_hip_decode_tiff_batch: tiff_expand and tiff_convert, tiff_kernels.hip) against the host
decoder, which tests/test_tiff.py holds against the numpy restatement of the rules (tests/tiff_ref.py) and Pillow.
Every file a test lists as a device file is first asserted to be routed to the device (aeon_tiff_host_stage,
gpu_route == 1; tests/test_tiff_stage.py checks the same list on the CPU): none of the comparisons below can pass
through the host route.  The files come from tests/tiff_cases.py.  Then the decoder: windows of TIFF records, and one
that mixes all five containers.
"""
import functools
import os

import numpy as np
import pytest

import aeon_amd as A
from tests import tiff_cases as TC
from tests import tiff_ref as R
from tests import tiff_writer as W

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = [A.DECODE_BGR8, A.DECODE_GRAY8, A.DECODE_ANYDEPTH]
EDEVICE = -4


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = A.Context(0)
    yield c
    c.close()


def _decode(ctx, files, modes, sync=True):
    """One decode_tiff_batch call: the records as arrays.  Rows are padded (stride > width, so row starts take
    every alignment) and the buffer is pre-filled, so a store outside a row shows."""
    import torch
    descs, shapes, off = [], [], 0
    for b, m in zip(files, modes):
        w, h, _, eb2 = A.tiff_info(b)
        eb = eb2 if m == A.DECODE_ANYDEPTH else 1
        cn = 3 if m == A.DECODE_BGR8 else 1
        stride = w * cn * eb + 5 + (len(descs) % 3)
        descs.append(A.ImgDesc(offset=off, width=w, height=h, stride=stride, channels=cn, elem_bytes=eb))
        shapes.append((h, w, cn, eb, stride))
        off += (stride * h + 15) // 16 * 16 + (2 if len(descs) % 2 else 0) * 16
    dst = torch.full((max(off, 16),), 0x5A, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx.decode_tiff_batch(files, modes, descs, dst.data_ptr(), stream)
    if not sync:
        return None
    ctx.synchronize(stream)
    host = dst.cpu().numpy()
    out, end = [], 0
    for d, (h, w, cn, eb, stride) in zip(descs, shapes):
        assert np.all(host[end:d.offset] == 0x5A), "bytes written between records"
        rows = host[d.offset:d.offset + stride * h].reshape(h, stride)
        end = d.offset + stride * h
        assert np.all(rows[:, w * cn * eb:] == 0x5A), "bytes written past a row"
        a = np.ascontiguousarray(rows[:, :w * cn * eb])
        a = a.view(np.uint16) if eb == 2 else a
        out.append(a.reshape(h, w, 3) if cn == 3 else a.reshape(h, w))
    assert np.all(host[end:] == 0x5A), "bytes written past the last record"
    return out


@functools.lru_cache(None)
def _expected(group):
    """(name, file, mode, the host decoder's record) of every file x mode of a group, computed once."""
    out = []
    for name, f in getattr(TC, group)():
        for m in MODES:
            want = A.decode_tiff(f, m)
            want.setflags(write=False)
            out.append((name, f, m, want))
    return out


def _check(res, exp):
    assert len(res) == len(exp)
    for r, (name, _, m, want) in zip(res, exp):
        assert r.dtype == want.dtype and r.shape == want.shape, (name, m)
        assert np.array_equal(r, want), (name, m, np.argwhere(r != want)[:3].tolist())


def _assert_routed(exp):
    for name, f, m, _ in exp:
        assert A.tiff_host_stage(f, m) == (True, len(f)), (name, "not routed to the device")


def test_device_files_alone_three_times(ctx):
    """Every device file x three modes in one call; and again (the second staging set, then the first reused)."""
    exp = _expected("device_files")
    _assert_routed(exp)
    files, modes = [e[1] for e in exp], [e[2] for e in exp]
    for _ in range(3):
        _check(_decode(ctx, files, modes), exp)


def test_mixed_call_with_host_routed_files(ctx):
    dev, hst = _expected("device_files")[::9], _expected("host_files")
    _assert_routed(dev)
    for name, f, m, _ in hst:
        assert A.tiff_host_stage(f, m)[0] is False, name
    exp = [e for pair in zip(dev, hst) for e in pair] + dev[len(hst):]
    for _ in range(2):
        _check(_decode(ctx, [e[1] for e in exp], [e[2] for e in exp]), exp)


def test_fixtures_from_pillow(ctx):
    FX = np.load(os.path.join(HERE, "golden", "tiff_fixtures.npz"))
    # (Pillow writes its RGBA files with unassociated alpha: refused, tests/test_tiff.py asserts how)
    names = sorted(k[:-5] for k in FX.files if k.endswith(".file") and "_RGBA_" not in k)
    assert len(names) == 40
    exp = [(n, FX[n + ".file"].tobytes(), m, A.decode_tiff(FX[n + ".file"].tobytes(), m)) for n in names for m in MODES]
    dev = [e for e in exp if A.tiff_host_stage(e[1], e[2])[0]]
    assert len(dev) >= len(exp) // 2
    _check(_decode(ctx, [e[1] for e in exp], [e[2] for e in exp]), exp)


def test_refused_file_refuses_the_call_before_any_launch(ctx):
    import torch
    good = W.write(np.full((4, 4), 7, np.uint8), 1, "lzw")
    bad = W.write(np.full((4, 4), 7, np.uint8), 1, 7)  # JPEG-in-TIFF
    with pytest.raises(A.AeonHipError) as e0:
        A.decode_tiff(bad)
    descs = [A.ImgDesc(offset=64 * i, width=4, height=4, stride=4, channels=1, elem_bytes=1) for i in range(2)]
    dst = torch.full((128,), 0x5A, dtype=torch.uint8, device="cuda")
    with pytest.raises(A.AeonHipError) as e1:
        ctx.decode_tiff_batch([good, bad], [A.DECODE_GRAY8] * 2, descs, dst.data_ptr(), 0)
    assert (e1.value.code, str(e1.value)) == (e0.value.code, str(e0.value))
    ctx.synchronize(0)
    assert bool((dst == 0x5A).all()), "a refused call wrote"
    assert np.array_equal(_decode(ctx, [good], [A.DECODE_GRAY8])[0], np.full((4, 4), 7))  # the context is usable


@pytest.mark.parametrize("case", range(5))
def test_corrupt_strip_is_a_device_error_and_the_context_goes_on(ctx, case):
    """Corrupt data in a sound file: nothing the host half can see, the wave that decodes the strip refuses it."""
    import torch
    name, f = TC.corrupt_files()[case]
    assert A.tiff_host_stage(f, A.DECODE_BGR8) == (True, len(f)), name  # (the host half decodes nothing of a routed file)
    good = _expected("device_files")[3:40:6]
    _assert_routed(good)
    _decode(ctx, [f, good[0][1]], [A.DECODE_BGR8, good[0][2]], sync=False)
    with pytest.raises(A.AeonHipError) as e:
        ctx.synchronize(torch.cuda.current_stream().cuda_stream)
    assert e.value.code == EDEVICE and "TIFF" in str(e.value), (name, str(e.value))
    _check(_decode(ctx, [e[1] for e in good], [e[2] for e in good]), good)


# ---- the decoder: C5 records (image + mask) whose files the TIFF stage decodes ----------------------------------
IMG64 = dict(height=64, width=64, type="image", channels=3, output_type="float", channel_major=True, bgr_to_rgb=True)
MSK64 = dict(height=64, width=64, type="pixelmask", channels=1, output_type="uint8_t")


def _c5_window(seed, n=6):
    """n records 64..120 a side: an RGB TIFF image (LZW + predictor 2, Deflate, PackBits or uncompressed by turns)
    and a 16-bit gray TIFF mask (the depth-map pairing), with each file's decode by the reference."""
    rng = np.random.default_rng(seed)
    recs, decoded = [], []
    for i in range(n):
        w, h = int(rng.integers(64, 121)), int(rng.integers(64, 121))
        img = A.synthetic_image(700 + 10 * seed + i, w, h, 3)  # BGR
        cls = np.kron(rng.integers(0, 5, (8, 8)), np.ones((16, 16), np.int64))[:h, :w]
        comp = ["lzw", "deflate", "packbits", "raw"][i % 4]
        ifile = W.write(img[:, :, ::-1], 2, comp, pred=2 if comp in ("lzw", "deflate") else 1, rps=[8, 16, 5, None][i % 4], big=bool(i & 1))
        mfile = W.write((cls * 9700 + i * 13 + (np.arange(w) % 7)).astype(np.uint16), 1, ["deflate", "lzw"][i % 2], pred=2,
                        rps=16, big=not (i & 1), pad=i)
        # (the decoder keeps a Deflate file whose strips hold more than a third of its samples on the host pool: these
        # noisy images, not the blob masks -- both routes in every window; the batch call alone takes either)
        assert A.tiff_decoder_route(ifile) is (comp != "deflate") and A.tiff_decoder_route(mfile)
        assert A.tiff_host_stage(ifile)[0] and A.tiff_host_stage(mfile, A.DECODE_ANYDEPTH)[0]
        recs.append((ifile, mfile))
        decoded.append((R.decode(ifile, R.BGR8), R.decode(mfile, R.ANYDEPTH)))
        assert np.array_equal(decoded[-1][0], img) and decoded[-1][1].dtype == np.uint16
    return recs, decoded


def _c5_oracle(decoded, params):
    from aeon_amd import configs as C
    from tests import helpers as H
    ref_img = np.stack(H.oracle_records([r[0] for r in decoded], params, C.out_desc_for(IMG64, C.C5_AUG)))
    mod, masks = C.out_desc_for(MSK64, C.C5_AUG), []
    for r, p in zip(decoded, params):
        m = r[1]  # saturate_cast<uchar> of the 16-bit NEAREST result
        lo = H.oracle_records([(m & 0xff).astype(np.uint8)], [p], mod, mask=True)[0]
        hi = H.oracle_records([(m >> 8).astype(np.uint8)], [p], mod, mask=True)[0]
        masks.append(np.minimum(hi.astype(np.uint32) * 256 + lo, 255).astype(np.uint8))
    return ref_img, masks


def _c5_cfg(n):
    from aeon_amd import configs as C
    return dict(batch_size=n, random_seed=4, etl=[IMG64, MSK64], augmentation=[C.C5_AUG])


def test_decoder_c5_tiff_records_decode():
    recs, decoded = _c5_window(1)
    sizes = [(r[0].shape[1], r[0].shape[0]) for r in decoded]
    params = A.Decoder(_c5_cfg(len(recs))).draw_params(sizes)
    img, msk = A.Decoder(_c5_cfg(len(recs))).decode(recs)
    ref_img, ref_msk = _c5_oracle(decoded, params)
    assert np.array_equal(img, ref_img)
    for i, want in enumerate(ref_msk):
        assert np.array_equal(msk[i], want.reshape(msk[i].shape)), i


def test_decoder_c5_tiff_records_three_windows_submit_wait():
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


def test_decoder_one_window_mixing_jpeg_png_ppm_bmp_and_tiff():
    """Image records of all five containers (and a TIFF of the host route) in one window: the JPEG, the PNG, the PPM and
    the BMP take the paths they took before the stage existed."""
    from aeon_amd import configs as C
    from oracle import png_oracle as PO
    from tests import helpers as H
    from tests import pixmap_writer as PW2
    from tests import png_writer as PW
    jf = np.load(os.path.join(HERE, "golden", "jpeg_fixtures.npz"))
    recs, decoded = [], []
    for i in range(12):
        img = A.synthetic_image(40 + i, 70 + 5 * i, 66 + 3 * i, 3)
        if i % 6 == 0:
            name = "s420_q50" if i else "s422_q75"
            f, img = jf[name + ".jpg"].tobytes(), jf[name + ".bgr_px"]
        elif i % 6 == 1:
            f = PW.write(img[:, :, ::-1], 2, 8, (0, 1, 2, 3, 4))
            assert np.array_equal(PO.decode(f, PO.BGR8), img)
        elif i % 6 == 2:
            f = PW2.pnm(6, img[:, :, ::-1], 255, comment=2 + i)
        elif i % 6 == 3:
            f = PW2.bmp(img, 24, gap=i % 4)
        elif i % 6 == 4:
            f = W.write(img[:, :, ::-1], 2, "lzw", pred=2, rps=7, big=bool(i & 2))
            assert A.tiff_decoder_route(f) and np.array_equal(R.decode(f, R.BGR8), img)
        else:
            img = A.synthetic_image(40 + i, 160, 120, 3)
            f = W.write(img[:, :, ::-1], 2, "lzw")  # one strip above 32 KiB: the host route
            assert not A.tiff_decoder_route(f) and np.array_equal(R.decode(f, R.BGR8), img)
        recs.append((f,))
        decoded.append(img)
    cfg = dict(batch_size=len(recs), random_seed=9, etl=[IMG64], augmentation=[C.C5_AUG])
    params = A.Decoder(cfg).draw_params([(a.shape[1], a.shape[0]) for a in decoded])
    (got,) = A.Decoder(cfg).decode(recs)
    ref = np.stack(H.oracle_records(decoded, params, C.out_desc_for(IMG64, C.C5_AUG)))
    assert np.array_equal(got, ref)


def test_decoder_leaves_other_files_to_the_jpeg_parser():
    """What the strict sniff does not take gets the JPEG header parser's error, word for word: II with a wrong
    version, an IFD offset past the file, a BigTIFF."""
    import struct
    cfg = dict(batch_size=1, random_seed=0, etl=[IMG64])
    for f in [b"II" + struct.pack("<HI", 41, 8) + bytes(24), b"II" + struct.pack("<HI", 42, 400) + bytes(24),
              b"MM" + struct.pack(">HI", 42, 31) + bytes(24), b"II" + struct.pack("<HI", 43, 8) + bytes(24)]:
        with pytest.raises(A.AeonHipError) as e:
            A.jpeg_info(f)
        want = str(e.value).split(": ", 1)[1]
        with pytest.raises(Exception) as d:
            A.Decoder(cfg).decode([(f,)])
        assert want in str(d.value) and "TIFF" not in str(d.value), (f[:8], str(d.value))
    # a recognised TIFF that the host decoder refuses keeps the TIFF decoder's message
    with pytest.raises(Exception) as d:
        A.Decoder(cfg).decode([(W.write(np.zeros((64, 64), np.uint8), 1, 7),)])
    assert "TIFF: JPEG compression is not supported" in str(d.value)
