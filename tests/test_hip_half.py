"""GPU: float16 / bfloat16 image outputs.  Every element must be the float32 output's element rounded
once to nearest even (tests/half_ref.py on the oracle's float32 output), compared as 16-bit patterns:
the vectorised plane store and its dynamic tail, the generic per-element store, the rounding edges,
the two-launch photometric path with its per-record table, the pre-passes, the decoder, the pair call
and the stager -- and the refusals of everything that is not an image."""
import os

import numpy as np
import pytest

import aeon_amd as A
from aeon_amd import configs as C
from tests import half_ref as R
from tests import helpers as H

pytestmark = pytest.mark.gpu
TYPES = ["float16", "bfloat16"]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = A.Context(0)
    yield c
    c.close()


def _desc(name, cn=3, major=True, bgr=False, mean=None, stddev=None, w=0, h=0):
    return A.out_desc(channels=cn, channel_major=major, bgr_to_rgb=bgr, dtype=name, mean=mean, stddev=stddev,
                      item_stride=w * h * cn * (4 if name == "float32" else 2))


def _shape(out, p):
    return (out.channels, p.out_h, p.out_w) if out.channel_major else (p.out_h, p.out_w, out.channels)


def _run(ctx, imgs, params, out, offset=0):
    """The records' items as uint16 patterns; the items start `offset` bytes into the device buffer."""
    import torch
    arena, descs = A.pack_images(imgs)
    src = torch.from_numpy(arena).to("cuda")
    n = len(imgs)
    dst = torch.full((n * out.item_stride + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    assert dst.data_ptr() % 16 == 0
    stream = torch.cuda.current_stream().cuda_stream
    ctx.augment_batch(descs, src.data_ptr(), params, out, dst.data_ptr() + offset, stream)
    ctx.synchronize(stream)
    host = dst.cpu().numpy()
    res = []
    for i, p in enumerate(params):
        sh = _shape(out, p)
        at = offset + i * out.item_stride
        res.append(host[at: at + 2 * int(np.prod(sh))].copy().view(np.uint16).reshape(sh))
    # nothing outside the items was written (before the first, between short items, after the last)
    keep = np.ones(host.size, bool)
    for i, p in enumerate(params):
        at = offset + i * out.item_stride
        keep[at: at + 2 * int(np.prod(_shape(out, p)))] = False
    assert (host[keep] == 0xAB).all(), "bytes outside the items were written"
    return res


_ref_cache = {}


def _ref32(key, imgs, params, out):
    """The oracle's float32 records of the same output config, computed once per `key`."""
    if key not in _ref_cache:
        o32 = A.OutDesc.from_buffer_copy(out)
        o32.dtype = A.DTYPES["float32"][0]
        _ref_cache[key] = H.oracle_records(imgs, params, o32)
    return _ref_cache[key]


def _check(got, ref32, name, what):
    assert len(got) == len(ref32)
    for i, (g, r) in enumerate(zip(got, ref32)):
        want = R.half_bits(r, name)
        assert g.shape == want.shape, (what, name, i)
        if not np.array_equal(g, want):
            bad = np.argwhere(g != want)
            k = tuple(bad[0])
            raise AssertionError(f"{what} {name}: record {i} differs at {len(bad)} of {g.size} elements, first {list(k)}: "
                                 f"got {g[k]:#06x}, want {want[k]:#06x} (float32 {r[k]!r})")


def _crops(n, srcs, ow, oh, seed):
    """n records over the source sizes in turn: full frames and random crops, flip alternating."""
    rng = np.random.default_rng(seed)
    imgs, params = [], []
    for i in range(n):
        w, h = srcs[i % len(srcs)]
        imgs.append(A.synthetic_image(1000 * seed + i, w, h, 3))
        if i % 3 == 0:
            cx, cy, cw, ch = 0, 0, w, h
        else:
            cw, ch = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
            cx, cy = int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1))
        params.append(A.aug_params(crop_x=cx, crop_y=cy, crop_w=cw, crop_h=ch, out_w=ow, out_h=oh, flip=(i // 2) % 2))
    return imgs, params


SRCS = [(7, 5), (64, 48), (300, 200), (31, 90)]


# ---- 1. the vector form ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("bgr,mean", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("ow,oh", [(4, 1), (8, 3), (60, 5), (224, 33)])
def test_vector_form(ctx, ow, oh, bgr, mean):
    """CHW planes, widths % 4 == 0, aligned items: one 8-byte store per lane and plane row.  224 x 33 is two
    32-row bands; sources from 7 x 5 (upscaled) to 300 x 200, flip on and off."""
    imgs, params = _crops(8, SRCS, ow, oh, seed=ow + oh)
    kw = dict(bgr=bgr, mean=C.MEAN if mean else None, stddev=C.STDDEV if mean else None, w=ow, h=oh)
    for name in TYPES:
        out = _desc(name, **kw)
        # items 16-byte aligned: pad the stride where the item is not a multiple of 16 bytes
        out.item_stride = (out.item_stride + 15) // 16 * 16
        ref = _ref32(("vec", ow, oh, bgr, mean), imgs, params, out)
        _check(_run(ctx, imgs, params, out), ref, name, f"vector {ow}x{oh}")


# ---- 2. the persistent grid's dynamic tail ---------------------------------------------------------------------
def test_dynamic_tail_thousand_records(ctx):
    """1,000 records of 8 x 4 output: more tiles than the 768 workgroups of a full grid, so the last rounds
    are handed out by the counter.  Every record is checked."""
    n = 1000
    imgs, params = _crops(n, [(12, 9), (9, 14), (16, 8)], 8, 4, seed=2)
    for name in TYPES:
        out = _desc(name, bgr=True, mean=C.MEAN, stddev=C.STDDEV, w=8, h=4)
        ref = _ref32("tail", imgs, params, out)
        _check(_run(ctx, imgs, params, out), ref, name, "tail")


# ---- 3. the generic form ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["hwc", "w5", "w7", "gray", "offset2", "mixed"])
def test_generic_form(ctx, case):
    """Everything the vector form does not take: HWC items, widths that are no multiple of 4, one-channel
    images, items that are not 16-byte aligned, and a batch whose widths differ (one of them odd)."""
    ow, oh, cn, major, offset = 12, 6, 3, True, 0
    if case == "hwc":
        major = False
    elif case in ("w5", "w7"):
        ow = int(case[1])
    elif case == "gray":
        cn = 1
    elif case == "offset2":
        offset = 2
    imgs, params = _crops(6, SRCS, ow, oh, seed=len(case) + ow)
    if case == "gray":
        imgs = [np.ascontiguousarray(im[:, :, 1]) for im in imgs]
    if case == "mixed":
        for p, w in zip(params, (12, 6, 8, 5, 12, 4)):
            p.out_w = w
    mean = C.MEAN[:cn]
    for name in TYPES:
        out = _desc(name, cn=cn, major=major, bgr=(cn == 3), mean=mean, stddev=C.STDDEV[:cn], w=ow, h=oh)
        out.item_stride = (out.item_stride + 15) // 16 * 16
        ref = _ref32(("gen", case), imgs, params, out)
        _check(_run(ctx, imgs, params, out, offset), ref, name, case)


# ---- 4. rounding edges through the kernel ----------------------------------------------------------------------
def _all_values_image():
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    return np.ascontiguousarray(np.stack([v, 255 - v, (v.astype(np.int32) * 7 % 256).astype(np.uint8)], axis=2))


M128 = float(np.float32(128.0 / 255.0)) + 3e-5
M51 = float(np.float32(float(np.float32(51.0)) * (1.0 / 255.0)))  # the standardize chain's x/255 for x = 51


@pytest.mark.parametrize("case,mean,stddev", [("integers", None, None), ("subnormal", [M128] * 3, [1.0] * 3),
                                              ("inf", C.MEAN, [1e-6] * 3), ("zeros", [M51] * 3, [-1.0] * 3)])
@pytest.mark.parametrize("ow", [16, 15])
def test_rounding_edges(ctx, case, mean, stddev, ow):
    """All 256 values of every channel with identity geometry (width 16: the vector store; a 15-wide crop:
    the generic one) through LUTs that land on exact integers, float16 subnormals, +-inf in float16 (finite in
    bfloat16) and zeros of both signs.  No clamping, no flush to zero."""
    img = _all_values_image()
    params = [A.aug_params(crop_x=0, crop_y=0, crop_w=ow, crop_h=16, out_w=ow, out_h=16, flip=f) for f in (0, 1)]
    imgs = [img, img]
    seen = {}
    for name in TYPES:
        out = _desc(name, mean=mean, stddev=stddev, w=ow, h=16)
        out.item_stride = (out.item_stride + 15) // 16 * 16
        ref = _ref32(("edge", case, ow), imgs, params, out)
        _check(_run(ctx, imgs, params, out), ref, name, f"{case} w{ow}")
        seen[name] = R.half_bits(ref[0], name)
    # the case is what it says (of the reference: the kernel was compared with it above)
    f16, b16 = seen["float16"], seen["bfloat16"]
    if case == "integers":
        assert set(f16.view(np.float16).astype(np.float32).reshape(-1).tolist()) >= set(map(float, range(256)))
    if case == "subnormal":
        assert (((f16 & 0x7C00) == 0) & ((f16 & 0x03FF) != 0)).any(), "no float16 subnormal in the reference"
    if case == "inf":
        assert (f16 == 0x7C00).any() and (f16 == 0xFC00).any(), "no +-inf in the float16 reference"
        assert ((b16 & 0x7F80) != 0x7F80).all(), "the bfloat16 reference must stay finite"
    if case == "zeros":
        z = np.concatenate([f16.reshape(-1), b16.reshape(-1)])
        assert (z == 0x8000).any(), "no negative zero in the reference"


# ---- 5. the photometric chain: two launches and the per-record table --------------------------------------------
def test_photometric_two_launch_path():
    """C3-style records (brightness, saturation, hue, contrast, lighting): contrast's pass 1, then the final
    pass reading the per-record f32 table and converting at the store.  The same batch on a context with
    AEON_HIP_RECORDS=0 (no single-launch record kernel, which stays float32-only) must give the same."""
    sizes = [(40, 30), (33, 47), (64, 64), (25, 25), (80, 20)]
    imgs = [A.synthetic_image(70 + i, w, h, 3) for i, (w, h) in enumerate(sizes)]
    params = H.draw_params(C.C3_AUG, sizes, 16, 16, seed=5)
    assert any(p.contrast != 1.0 for p in params) and any(p.n_lighting == 3 for p in params)
    old = os.environ.get("AEON_HIP_RECORDS")
    res = {}
    for rec in ("default", "0"):
        if rec == "0":
            os.environ["AEON_HIP_RECORDS"] = "0"
        try:
            c = A.Context(0)
        finally:
            if rec == "0":
                if old is None:
                    del os.environ["AEON_HIP_RECORDS"]
                else:
                    os.environ["AEON_HIP_RECORDS"] = old
        try:
            for name in TYPES:
                out = _desc(name, bgr=True, mean=C.MEAN, stddev=C.STDDEV, w=16, h=16)
                res[rec, name] = _run(c, imgs, params, out)
                _check(res[rec, name], _ref32("photo", imgs, params, out), name, f"C3 records={rec}")
        finally:
            c.close()
    for name in TYPES:
        assert all(np.array_equal(a, b) for a, b in zip(res["default", name], res["0", name]))


# ---- 6. the pre-passes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cubic", "rotate30", "expand", "resize_short"])
def test_pre_passes(ctx, case):
    """One record each into a 12 x 8 item behind a pre-pass: a CUBIC resize (which writes float32 items
    itself, so here the tile kernel's copy pass follows it), a rotation, an SSD expand canvas, resize_short."""
    w, h = 40, 30
    img = A.synthetic_image(90 + len(case), w, h, 3)
    kw = dict(crop_x=3, crop_y=2, crop_w=30, crop_h=24, out_w=12, out_h=8, flip=1)
    if case == "cubic":
        kw["interp"] = A.INTERP_CUBIC
    elif case == "rotate30":
        kw["angle"] = 30
    elif case == "expand":
        kw.update(expand_ratio=2.0, expand_x=17, expand_y=9, expand_w=2 * w, expand_h=2 * h, crop_x=10, crop_y=5,
                  crop_w=50, crop_h=40)
    elif case == "resize_short":
        kw.update(resize_short_size=20, crop_x=2, crop_y=2, crop_w=16, crop_h=16)
    params = [A.aug_params(**kw)]
    for name in TYPES:
        out = _desc(name, bgr=True, mean=C.MEAN, stddev=C.STDDEV, w=12, h=8)
        _check(_run(ctx, [img], params, out), _ref32(("pre", case), [img], params, out), name, case)


# ---- 7. the decoder ---------------------------------------------------------------------------------------------
def _jpeg_records(n):
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "jpeg_fixtures.npz"))
    names = sorted({k.rsplit(".", 1)[0] for k in fx.files})[:n]
    return [fx[k + ".jpg"].tobytes() for k in names]


@pytest.mark.parametrize("batch_major", [True, False])
def test_decoder_float16_image_and_label(batch_major):
    """An image + label config with float16 and mean / stddev over three encoded JPEG records: decode() into
    host arrays (batch_major false: each batch transposed by the 2-byte element), then submit / wait into
    device buffers."""
    import torch

    import oracle as O
    files = _jpeg_records(3)
    etl = [{"type": "image", "height": 24, "width": 32, "channels": 3, "output_type": "float16", "channel_major": True,
            "bgr_to_rgb": True, "extended_output_type": True}, {"type": "label", "binary": False}]
    cfg = dict(batch_size=3, random_seed=11, etl=etl, augmentation=[C.C2_AUG], batch_major=batch_major)
    recs = [(f, str(4 + i)) for i, f in enumerate(files)]
    d = A.Decoder(cfg)
    assert d.outputs[0]["type_name"] == "float16" and d.outputs[0]["item_bytes"] == 2 * 3 * 24 * 32
    dec = [O.jpeg_decode(f, 3) for f in files]
    params = H.draw_params(C.C2_AUG, [(x.shape[1], x.shape[0]) for x in dec], 32, 24, seed=11)
    o32 = C.out_desc_for(dict(etl[0], output_type="float"), C.C2_AUG)
    want = np.stack([R.f16_bits(r) for r in H.oracle_records(dec, params, o32)])
    item = want[0].size
    if not batch_major:
        want = O.transpose(want.reshape(-1).view(np.uint8), 3, item, 2).view(np.uint16)
    img, lab = d.decode(recs)
    assert img.dtype == np.float16
    assert np.array_equal(img.view(np.uint16).reshape(-1), want.reshape(-1))
    assert lab.reshape(-1).tolist() == [4, 5, 6]
    # the same window, double-buffered, into device memory
    d2 = A.Decoder(cfg)
    bufs = [torch.zeros(3 * o["item_bytes"], dtype=torch.uint8, device="cuda") for o in d2.outputs]
    enc = d2.encoded(recs)
    d2.submit(enc, [b.data_ptr() for b in bufs], on_device=True)
    d2.wait()
    got = bufs[0].cpu().numpy().view(np.uint16)
    assert np.array_equal(got, want.reshape(-1))
    t = A.as_torch(bufs[0].cpu().numpy().view(np.float16), d2.outputs[0]["type_name"])
    assert t.dtype == torch.float16


# ---- 8. the pair call -------------------------------------------------------------------------------------------
def test_pair_batch_half_image_and_refused_half_mask(ctx):
    import torch
    n = 4
    rng = np.random.default_rng(8)
    imgs = [A.synthetic_image(i, 40, 30, 3) for i in range(n)]
    masks = [rng.integers(0, 21, (30, 40), dtype=np.uint8) for _ in range(n)]
    aug = {"type": "image", "center": False, "scale": [0.5, 1.0], "flip_enable": True}
    params = H.draw_params(aug, [(40, 30)] * n, 16, 16, seed=8)
    iout = _desc("float16", bgr=True, mean=C.MEAN, stddev=C.STDDEV, w=16, h=16)
    mout = A.out_desc(channels=1, dtype="uint8", item_stride=16 * 16)
    ia, idescs = A.pack_images(imgs)
    ma, mdescs = A.pack_images(masks)
    isrc, msrc = torch.from_numpy(ia).to("cuda"), torch.from_numpy(ma).to("cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(mo):
        idst = torch.full((n * iout.item_stride,), 0xAB, dtype=torch.uint8, device="cuda")
        mdst = torch.full((n * 16 * 16 * 2,), 0xCD, dtype=torch.uint8, device="cuda")
        try:
            ctx.pair_batch(idescs, isrc.data_ptr(), mdescs, msrc.data_ptr(), params, iout, idst.data_ptr(), mo,
                           mdst.data_ptr(), stream)
        finally:
            ctx.synchronize(stream)
        return idst.cpu().numpy(), mdst.cpu().numpy()

    ih, mh = call(mout)
    got = [ih[i * iout.item_stride:(i + 1) * iout.item_stride].view(np.uint16).reshape(3, 16, 16) for i in range(n)]
    _check(got, _ref32("pair", imgs, params, iout), "float16", "pair image")
    mref = H.oracle_records(masks, params, mout, mask=True)
    for i in range(n):
        assert np.array_equal(mh[i * 256:(i + 1) * 256].reshape(1, 16, 16), mref[i]), i
    assert (mh[n * 256:] == 0xCD).all()
    # the mask as float16: refused before anything is launched -- neither output is touched
    for name in TYPES:
        bad = A.out_desc(channels=1, dtype=name, item_stride=16 * 16 * 2)
        idst = torch.full((n * iout.item_stride,), 0xAB, dtype=torch.uint8, device="cuda")
        mdst = torch.full((n * 16 * 16 * 2,), 0xCD, dtype=torch.uint8, device="cuda")
        with pytest.raises(A.AeonHipError) as e:
            ctx.pair_batch(idescs, isrc.data_ptr(), mdescs, msrc.data_ptr(), params, iout, idst.data_ptr(), bad,
                           mdst.data_ptr(), stream)
        ctx.synchronize(stream)
        assert e.value.code == A.AEON_HIP_EUNSUPPORTED and name in str(e.value)
        assert (idst.cpu().numpy() == 0xAB).all() and (mdst.cpu().numpy() == 0xCD).all()


@pytest.mark.parametrize("name", TYPES)
def test_mask_paths_and_canvas_refuse_half(ctx, name):
    """aeon_hip_mask_batch, aeon_hip_depthmap_batch, a MASK stager and fixed_aspect_ratio: EUNSUPPORTED
    naming the type, and no byte written."""
    import torch
    mask = np.arange(30 * 40, dtype=np.uint8).reshape(30, 40)
    arena, descs = A.pack_images([mask])
    src = torch.from_numpy(arena).to("cuda")
    p = [A.aug_params(crop_x=0, crop_y=0, crop_w=40, crop_h=30, out_w=16, out_h=16)]
    out = A.out_desc(channels=1, dtype=name, item_stride=16 * 16 * 2)
    stream = torch.cuda.current_stream().cuda_stream
    for fn in (ctx.mask_batch, ctx.depthmap_batch):
        dst = torch.full((16 * 16 * 2,), 0xCD, dtype=torch.uint8, device="cuda")
        with pytest.raises(A.AeonHipError) as e:
            fn(descs, src.data_ptr(), p, out, dst.data_ptr(), stream)
        ctx.synchronize(stream)
        assert e.value.code == A.AEON_HIP_EUNSUPPORTED and name in str(e.value)
        assert (dst.cpu().numpy() == 0xCD).all()
    with pytest.raises(A.AeonHipError) as e:
        A.Stager(ctx, out, 2, A.STAGER_MASK)
    assert e.value.code == A.AEON_HIP_EUNSUPPORTED and name in str(e.value)
    # an image into a fixed_aspect_ratio canvas
    img = A.synthetic_image(3, 40, 30, 3)
    arena, descs = A.pack_images([img])
    src = torch.from_numpy(arena).to("cuda")
    far = A.out_desc(channels=3, dtype=name, item_stride=16 * 16 * 3 * 2, fixed_aspect_ratio=True, canvas=(16, 16))
    dst = torch.full((16 * 16 * 3 * 2,), 0xCD, dtype=torch.uint8, device="cuda")
    with pytest.raises(A.AeonHipError) as e:
        ctx.augment_batch(descs, src.data_ptr(), [A.aug_params(crop_x=0, crop_y=0, crop_w=40, crop_h=30, out_w=16, out_h=12)],
                          far, dst.data_ptr(), stream)
    ctx.synchronize(stream)
    assert e.value.code == A.AEON_HIP_EUNSUPPORTED and name in str(e.value) and "fixed_aspect_ratio" in str(e.value)
    assert (dst.cpu().numpy() == 0xCD).all()


# ---- 9. the stager ----------------------------------------------------------------------------------------------
def test_stager_window_float16(ctx):
    """One window of a stager whose output desc is float16: staged records, one flush, the batch buffer."""
    n = 4
    sizes = [(50, 40), (64, 48), (33, 70), (40, 40)]
    imgs = [A.synthetic_image(200 + i, w, h, 3) for i, (w, h) in enumerate(sizes)]
    aug = dict(C.C2_AUG)
    params = H.draw_params(aug, sizes, 20, 12, seed=9)
    out = _desc("float16", bgr=True, mean=C.MEAN, stddev=C.STDDEV, w=20, h=12)
    st = A.Stager(ctx, out, n)
    buf = np.full(n * out.item_stride, 0xAB, np.uint8)
    try:
        for i in range(n):
            st.stage(buf.ctypes.data, i, imgs[i], params[i])
        st.flush(buf.ctypes.data)
    finally:
        st.close()
    got = [buf[i * out.item_stride:(i + 1) * out.item_stride].view(np.uint16).reshape(3, 12, 20) for i in range(n)]
    _check(got, _ref32("stager", imgs, params, out), "float16", "stager")
