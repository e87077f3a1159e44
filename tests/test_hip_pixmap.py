"""GPU: the pixmap stage (aeon_hip_decode_pixmap_batch: pixmap_convert, pixmap_kernels.hip) against the numpy
restatement of the decode rules (tests/pixmap_ref.py) and the host decoder.  Every file a test lists as a device
file is first asserted to be routed to the device (aeon_pixmap_host_stage, gpu_route == 1;
tests/test_pixmap_stage.py checks the same list on the CPU): none of the comparisons below can pass through the
host route.  The files come from tests/pixmap_cases.py.  Then the decoder: windows of PNM and BMP records, and one
that mixes all four containers.
"""
import functools
import os

import numpy as np
import pytest

import aeon_amd as A
from tests import pixmap_cases as PC
from tests import pixmap_ref as R
from tests import pixmap_writer as W

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = [A.DECODE_BGR8, A.DECODE_GRAY8, A.DECODE_ANYDEPTH]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = A.Context(0)
    yield c
    c.close()


def _decode(ctx, files, modes):
    """One decode_pixmap_batch call: the records as arrays.  Rows are padded (stride > width, so row starts take
    every alignment) and the buffer is pre-filled, so a store outside a row shows."""
    import torch
    descs, shapes, off = [], [], 0
    for b, m in zip(files, modes):
        w, h, d, _, _ = A.pixmap_info(b)
        eb = 2 if (m == A.DECODE_ANYDEPTH and d == 16) else 1
        cn = 3 if m == A.DECODE_BGR8 else 1
        stride = w * cn * eb + 5 + (len(descs) % 3)
        descs.append(A.ImgDesc(offset=off, width=w, height=h, stride=stride, channels=cn, elem_bytes=eb))
        shapes.append((h, w, cn, eb, stride))
        off += (stride * h + 15) // 16 * 16 + (2 if len(descs) % 2 else 0) * 16
    dst = torch.full((max(off, 16),), 0x5A, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx.decode_pixmap_batch(files, modes, descs, dst.data_ptr(), stream)
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
    """(name, file, mode, reference decode) of every file x mode of a group, computed once; the host decoder agrees."""
    out = []
    for name, f in getattr(PC, group)():
        for m in MODES:
            want = R.decode(f, m)
            host = A.decode_pixmap(f, m)
            assert host.dtype == want.dtype and np.array_equal(host, want), (name, m)
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
        assert A.pixmap_host_stage(f, m) == (True, len(f)), (name, "not routed to the device")


def test_device_files_alone_twice(ctx):
    """Every device file x three modes in one call; and again (the second staging set, then the first reused)."""
    exp = _expected("device_files")
    _assert_routed(exp)
    files, modes = [e[1] for e in exp], [e[2] for e in exp]
    for _ in range(3):
        _check(_decode(ctx, files, modes), exp)


def test_mixed_call_with_host_routed_ascii_files(ctx):
    dev, asc = _expected("device_files")[::4], _expected("ascii_files")
    _assert_routed(dev)
    for name, f, m, _ in asc:
        assert A.pixmap_host_stage(f, m)[0] is False, name
    exp = [e for pair in zip(dev, asc) for e in pair] + dev[len(asc):] + asc[len(dev):]
    for _ in range(2):
        _check(_decode(ctx, [e[1] for e in exp], [e[2] for e in exp]), exp)


def test_fixtures_pillow_pins(ctx):
    FX = np.load(os.path.join(HERE, "golden", "pixmap_fixtures.npz"))
    keys = [(k.rsplit(".", 1)[0], k.rsplit(".", 1)[1]) for k in FX.files if not k.endswith(".file")]
    mode = dict(bgr8=A.DECODE_BGR8, gray8=A.DECODE_GRAY8, any=A.DECODE_ANYDEPTH)
    files = [FX[n + ".file"].tobytes() for n, _ in keys]
    for f, (n, k) in zip(files, keys):
        assert A.pixmap_host_stage(f, mode[k])[0], n
    res = _decode(ctx, files, [mode[k] for _, k in keys])
    for r, (n, k) in zip(res, keys):
        assert r.dtype == FX[n + "." + k].dtype and np.array_equal(r, FX[n + "." + k]), (n, k)


def test_refused_file_refuses_the_call_before_any_launch(ctx):
    import torch
    good = W.pnm(5, np.full((4, 4), 7), 255)
    bad = good[:-1]
    with pytest.raises(A.AeonHipError) as e0:
        A.decode_pixmap(bad)
    descs = [A.ImgDesc(offset=64 * i, width=4, height=4, stride=4, channels=1, elem_bytes=1) for i in range(2)]
    dst = torch.full((128,), 0x5A, dtype=torch.uint8, device="cuda")
    with pytest.raises(A.AeonHipError) as e1:
        ctx.decode_pixmap_batch([good, bad], [A.DECODE_GRAY8] * 2, descs, dst.data_ptr(), 0)
    assert (e1.value.code, str(e1.value)) == (e0.value.code, str(e0.value))
    ctx.synchronize(0)
    assert bool((dst == 0x5A).all()), "a refused call wrote"
    assert np.array_equal(_decode(ctx, [good], [A.DECODE_GRAY8])[0], np.full((4, 4), 7))  # the context is usable


# ---- the decoder: C5 records (image + mask) whose files the pixmap stage decodes ---------------------------------
IMG64 = dict(height=64, width=64, type="image", channels=3, output_type="float", channel_major=True, bgr_to_rgb=True)
MSK64 = dict(height=64, width=64, type="pixelmask", channels=1, output_type="uint8_t")


def _c5_window(seed, kind, n=6):
    """n records 64..120 a side.  kind "pnm": a P6 image and a 16-bit P5 mask (the depth-map pairing); "bmp": a
    24- or 32-bit BMP image and an 8-bit palette BMP mask.  With each file's decode by the reference."""
    rng = np.random.default_rng(seed)
    recs, decoded = [], []
    for i in range(n):
        w, h = int(rng.integers(64, 121)), int(rng.integers(64, 121))
        img = A.synthetic_image(900 + 10 * seed + i, w, h, 3)  # BGR
        cls = np.kron(rng.integers(0, 5, (8, 8)), np.ones((16, 16), np.int64))[:h, :w]
        if kind == "pnm":
            ifile = W.pnm(6, img[:, :, ::-1], 255, comment=2 + i)
            mfile = W.pnm(5, cls * 9700 + i * 13 + (np.arange(w) % 7), 65535, comment=3 + i)
        else:
            ifile = (W.bmp(np.dstack([img, img[:, :, :1]]), 32, header=108, top_down=True) if i % 2 else W.bmp(img, 24, gap=i % 4))
            pal = rng.integers(0, 256, (5 if i % 3 else 256, 3))
            mfile = W.bmp(cls + (i % 2) * (np.arange(w) % 3 == 0) * 3, 8, pal, top_down=bool(i % 2), gap=(i + 1) % 4)
        assert A.pixmap_host_stage(ifile, A.DECODE_BGR8)[0] and A.pixmap_host_stage(mfile, A.DECODE_ANYDEPTH)[0]
        recs.append((ifile, mfile))
        decoded.append((R.decode(ifile, R.BGR8), R.decode(mfile, R.ANYDEPTH)))
        assert np.array_equal(decoded[-1][0], img)
        assert decoded[-1][1].dtype == (np.uint16 if kind == "pnm" else np.uint8)
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


@pytest.mark.parametrize("kind", ["pnm", "bmp"])
def test_decoder_c5_pixmap_records_decode(kind):
    recs, decoded = _c5_window(1, kind)
    sizes = [(r[0].shape[1], r[0].shape[0]) for r in decoded]
    params = A.Decoder(_c5_cfg(len(recs))).draw_params(sizes)
    img, msk = A.Decoder(_c5_cfg(len(recs))).decode(recs)
    ref_img, ref_msk = _c5_oracle(decoded, params)
    assert np.array_equal(img, ref_img)
    for i, want in enumerate(ref_msk):
        assert np.array_equal(msk[i], want.reshape(msk[i].shape)), i


@pytest.mark.parametrize("kind", ["pnm", "bmp"])
def test_decoder_c5_pixmap_records_three_windows_submit_wait(kind):
    import torch
    wins = [_c5_window(s, kind) for s in (1, 2, 3)]
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


def test_decoder_one_window_mixing_jpeg_png_ppm_bmp_and_ascii():
    """Image records of all four containers (and an ASCII PPM, the host route) in one window: the JPEG and the PNG
    take the paths they took before the stage existed."""
    from aeon_amd import configs as C
    from oracle import png_oracle as PO
    from tests import helpers as H
    from tests import png_writer as PW
    jf = np.load(os.path.join(HERE, "golden", "jpeg_fixtures.npz"))
    recs, decoded = [], []
    for i in range(10):
        img = A.synthetic_image(40 + i, 70 + 5 * i, 66 + 3 * i, 3)
        if i % 5 == 0:
            name = "s420_q50" if i else "s422_q75"
            f, img = jf[name + ".jpg"].tobytes(), jf[name + ".bgr_px"]
        elif i % 5 == 1:
            f = PW.write(img[:, :, ::-1], 2, 8, (0, 1, 2, 3, 4))
            assert np.array_equal(PO.decode(f, PO.BGR8), img)
        elif i % 5 == 2:
            f = W.pnm(6, img[:, :, ::-1], 255, comment=2 + i)
        elif i % 5 == 3:
            f = W.bmp(img, 24, gap=i % 4)
        else:
            f = W.pnm(3, img[:, :, ::-1], 255)
        if i % 5 >= 2:
            assert A.pixmap_host_stage(f)[0] == (i % 5 != 4) and np.array_equal(R.decode(f, R.BGR8), img)
        recs.append((f,))
        decoded.append(img)
    cfg = dict(batch_size=len(recs), random_seed=9, etl=[IMG64], augmentation=[C.C5_AUG])
    params = A.Decoder(cfg).draw_params([(a.shape[1], a.shape[0]) for a in decoded])
    (got,) = A.Decoder(cfg).decode(recs)
    ref = np.stack(H.oracle_records(decoded, params, C.out_desc_for(IMG64, C.C5_AUG)))
    assert np.array_equal(got, ref)


def test_decoder_leaves_other_files_to_the_jpeg_parser():
    """What the strict sniff does not take gets the JPEG header parser's error, word for word: 16 bytes of zeros,
    a P7, a PNM magic without its whitespace byte, a BM with an info-header size the sniff refuses."""
    import struct
    cfg = dict(batch_size=1, random_seed=0, etl=[IMG64])
    for f in [bytes(16), b"P7\n" + bytes(13), b"P5x" + bytes(13), b"BM" + bytes(12) + struct.pack("<I", 20) + bytes(8)]:
        with pytest.raises(A.AeonHipError) as e:
            A.jpeg_info(f)
        want = str(e.value).split(": ", 1)[1]
        with pytest.raises(Exception) as d:
            A.Decoder(cfg).decode([(f,)])
        assert want in str(d.value) and "PNM" not in str(d.value) and "BMP" not in str(d.value), (f[:4], str(d.value))
    # a pixel mask may be a PNM or a BMP now; a JPEG mask keeps its message
    mcfg = dict(batch_size=1, random_seed=0, etl=[IMG64, MSK64])
    jf = np.load(os.path.join(HERE, "golden", "jpeg_fixtures.npz"))
    with pytest.raises(Exception) as d:
        A.Decoder(mcfg).decode([(jf["s444_rst.jpg"].tobytes(), jf["s444_rst.jpg"].tobytes())])
    assert "PNG files only" in str(d.value)
