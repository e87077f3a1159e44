"""image::rotate on the device (rotate_kernels.hip, rotate_tiles<CN>) at every integer angle and at the sizes
where its staging and its stores change path, bit for bit against the oracle.

rotate_tiles stages the source box of a 64 x 32 output tile in LDS (sized on the host per angle:
rot_box_words; error bit 64 where the box would not fit), through a 12-byte load for 4-pixel BGR groups inside
the image, byte loads for groups that straddle an edge, and zeros outside; it stores 4-pixel groups as 12 or
4 bytes where the output offset is aligned and bytewise otherwise.  Covered here:

  * every angle in [-180, 180) and 181 .. 359 (360 is the identity aeon never draws), one record each, for the
    four channel forms -- BGR bilinear (<3>), gray image bilinear (<1>), 8-bit mask nearest (<1>), 16-bit mask
    nearest (<2>) -- on a 150 x 100 source with the window 131 x 83 at (7, 5): 3 x 3 tiles with ragged last
    ones, output rows whose byte offsets alternate in alignment;
  * one angle per call at the angles whose box comes closest to the words the host grants (a call's LDS is
    sized by its steepest angle, so only a call of one angle runs that angle at its own bound);
  * sources of 1 .. 129 by 1 .. 65 pixels, whole-record windows, at the angles where rot_box_words peaks
    (26 / 27, 63 / 64), its tightest angle (240) and the axis and diagonal ones: 4-pixel staging groups that
    straddle both image edges at once, and the 12-byte load's `off + 12 <= stride * H` guard on the last row;
  * source rows padded by 1, 5 and 16 bytes (2, 6 and 16 for 16-bit records, whose stride must be even) of
    non-zero filler that must never reach an output;
  * rotate_tiles<0>, the form for a launch whose jobs differ in bytes per pixel.  aeon_hip_augment_batch refuses
    a batch that mixes 1- and 3-channel sources (asserted), and a pair call with rotation is two calls, so no
    image launch reaches it; a mask call that mixes 8-bit and 16-bit rotated masks does, and is run here.

Every output buffer starts as 0xAB, so a tile nobody wrote shows, and the bytes of an item past its record
must still be 0xAB afterwards; Context.synchronize raises if a kernel set a bit of the call's error word."""
import numpy as np
import pytest

import aeon_amd as A
from tests import helpers as H

pytestmark = pytest.mark.gpu

ALL_ANGLES = list(range(-180, 180)) + list(range(181, 360))
EDGE_ANGLES = [1, 26, 27, 45, 63, 64, 89, 90, 91, 135, 180, 240, 270, 333]
PAD_ANGLES = [-179, -135, -90, -64, -27, -1, 1, 26, 63, 120, 240, 333]
SRC_W, SRC_H = 150, 100
WINDOW = dict(crop_x=7, crop_y=5, crop_w=131, crop_h=83, out_w=131, out_h=83)
FORMS = ["bgr_bilinear", "gray_bilinear", "mask8_nearest", "mask16_nearest"]
FILL = 0xEE


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = A.Context(0)
    yield c
    c.close()


def source(form, seed, w, h):
    """A w x h record of the form's type: full-range bytes (uint16: two of them per element)."""
    if form == "bgr_bilinear":
        return A.synthetic_image(seed, w, h, 3)
    if form == "mask16_nearest":
        lo, hi = A.synthetic_image(seed, w, h, 1), A.synthetic_image(seed + 5000, w, h, 1)
        return (hi.astype(np.uint16) << 8) | lo
    return A.synthetic_image(seed, w, h, 1)


def pack(images, pad=0):
    """Records -> (uint8 arena, ImgDesc array), rows `pad` bytes longer than their pixels, the padding FILL."""
    chunks, descs, off = [], [], 0
    for im in images:
        eb = im.dtype.itemsize
        h, w = im.shape[:2]
        cn = 1 if im.ndim == 2 else im.shape[2]
        rows = np.ascontiguousarray(im, dtype="<u2" if eb == 2 else np.uint8).view(np.uint8).reshape(h, w * cn * eb)
        buf = np.full((h, w * cn * eb + pad), FILL, np.uint8)
        buf[:, :w * cn * eb] = rows
        tail = (-buf.size) % 16
        chunks += [buf.reshape(-1), np.full(tail, FILL, np.uint8)]
        descs.append(A.ImgDesc(offset=off, width=w, height=h, stride=buf.shape[1], channels=cn, elem_bytes=eb))
        off += buf.size + tail
    return np.concatenate(chunks), (A.ImgDesc * len(descs))(*descs)


def out_for(form, params):
    cn = 3 if form == "bgr_bilinear" else 1
    esz = 2 if form == "mask16_nearest" else 1
    most = max(p.out_w * p.out_h for p in params) * cn * esz
    return A.out_desc(channels=cn, channel_major=False, dtype="uint16" if esz == 2 else "uint8",
                      item_stride=(most + 15) // 16 * 16 + 16)


def rotate_on_device(ctx, form, images, params, pad=0):
    import torch
    arena, descs = pack(images, pad)
    out = out_for(form, params)
    src = torch.from_numpy(arena).to("cuda")
    dst = torch.full((len(images) * out.item_stride,), 0xAB, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    (ctx.augment_batch if form.endswith("bilinear") else ctx.mask_batch)(descs, src.data_ptr(), params, out, dst.data_ptr(),
                                                                        stream)
    ctx.synchronize(stream)  # (raises on error bit 64: a source box beyond the launch's LDS words)
    host = dst.cpu().numpy().reshape(len(images), out.item_stride)
    dt = A.NP_DTYPE[out.dtype]
    res = []
    for i, p in enumerate(params):
        nb = p.out_w * p.out_h * out.channels * np.dtype(dt).itemsize
        assert np.all(host[i, nb:] == 0xAB), f"record {i}: bytes written past the record"
        res.append(host[i, :nb].view(dt).reshape(p.out_h, p.out_w, out.channels))
    return res


def rotate_in_oracle(form, images, params):
    mask = not form.endswith("bilinear")
    o8 = A.out_desc(channels=3 if form == "bgr_bilinear" else 1, channel_major=False, dtype="uint8")
    if form != "mask16_nearest":
        return H.oracle_records(images, params, o8, mask=mask)
    # nearest moves whole elements: the 8-bit transform of the low and of the high byte plane, recombined
    lo = H.oracle_records([(m & 0xff).astype(np.uint8) for m in images], params, o8, mask=True)
    hi = H.oracle_records([(m >> 8).astype(np.uint8) for m in images], params, o8, mask=True)
    return [(b.astype(np.uint16) << 8) | a for a, b in zip(lo, hi)]


def check(ctx, form, images, params, what, pad=0):
    got = rotate_on_device(ctx, form, images, params, pad)
    ref = rotate_in_oracle(form, images, params)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape, (what, i, a.shape, b.shape)
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            at = tuple(bad[0])
            h, w = images[i].shape[:2]
            raise AssertionError(f"{what}: record {i} ({w} x {h}, angle {params[i].angle}): {len(bad)} values differ, "
                                 f"first at (y, x, c) = {at}: hip={a[at]} ref={b[at]}")


@pytest.mark.parametrize("form", FORMS)
def test_every_angle(ctx, form):
    """One call with a record per angle: the launch's LDS words are those of its steepest angle."""
    imgs = [source(form, 7 + (i & 3), SRC_W, SRC_H) for i in range(len(ALL_ANGLES))]
    params = [A.aug_params(angle=a, **WINDOW) for a in ALL_ANGLES]
    check(ctx, form, imgs, params, form + " every angle")


@pytest.mark.parametrize("form", ["bgr_bilinear", "mask8_nearest"])
def test_one_angle_per_launch(ctx, form):
    """A launch's LDS words are those of its steepest angle, so a call of many angles gives most of them room to
    spare: here every call holds one angle, whole-record windows (full 64 x 32 tiles), at the angles where the
    box comes closest to rot_box_words on the CPU (tests/test_rotation_box.py: 0.96 at +-60, +-120, 240, 300;
    0.959 at 79, 101, 259, 281), where rot_box_words peaks, and at the axis and diagonal ones."""
    im = source(form, 21, SRC_W, SRC_H)
    for a in (-120, -60, 1, 26, 27, 45, 54, 63, 64, 79, 90, 101, 120, 135, 180, 234, 240, 259, 270, 281, 300, 359):
        p = A.aug_params(crop_x=0, crop_y=0, crop_w=SRC_W, crop_h=SRC_H, out_w=SRC_W, out_h=SRC_H, angle=a)
        check(ctx, form, [im], [p], f"{form} alone at {a}")


@pytest.mark.parametrize("form", ["bgr_bilinear", "mask8_nearest"])
def test_small_and_edge_sizes(ctx, form):
    sizes = [(w, h) for w in (1, 2, 3, 4, 5, 63, 64, 65, 129) for h in (1, 2, 31, 32, 33, 65)]
    imgs, params = [], []
    for k, (w, h) in enumerate(sizes):
        im = source(form, 100 + k, w, h)
        for a in EDGE_ANGLES:
            imgs.append(im)
            params.append(A.aug_params(crop_x=0, crop_y=0, crop_w=w, crop_h=h, out_w=w, out_h=h, angle=a))
    check(ctx, form, imgs, params, form + " small sizes")


@pytest.mark.parametrize("pad", [1, 5, 16])
@pytest.mark.parametrize("form", FORMS)
def test_padded_source_rows(ctx, form, pad):
    if form == "mask16_nearest":
        pad = {1: 2, 5: 6, 16: 16}[pad]  # a 16-bit record's stride is even
    imgs = [source(form, 40 + i, SRC_W, SRC_H) for i in range(len(PAD_ANGLES))]
    params = [A.aug_params(angle=a, **WINDOW) for a in PAD_ANGLES]
    check(ctx, form, imgs, params, f"{form} stride + {pad}", pad=pad)


def test_mixed_channel_counts(ctx):
    """rotate_tiles<0>: refused for images (one channel count per call), reached by a mask call whose rotated
    records are 8-bit and 16-bit (1 and 2 bytes per pixel in one launch), into uint16 items."""
    import torch
    angles = [-150, -64, -27, 1, 45, 90, 120, 333]
    mixed = [source("bgr_bilinear" if i & 1 else "gray_bilinear", i, SRC_W, SRC_H) for i in range(len(angles))]
    params = [A.aug_params(angle=a, **WINDOW) for a in angles]
    arena, descs = pack(mixed)
    src = torch.from_numpy(arena).to("cuda")
    for cn in (1, 3):
        out = A.out_desc(channels=cn, channel_major=False, dtype="uint8", item_stride=131 * 83 * 3 + 7)
        dst = torch.zeros(len(mixed) * out.item_stride, dtype=torch.uint8, device="cuda")
        with pytest.raises(A.AeonHipError, match="decoded channels do not match the output config") as e:
            ctx.augment_batch(descs, src.data_ptr(), params, out, dst.data_ptr())
        assert e.value.code == A.AEON_HIP_EINVAL
    ctx.synchronize()
    masks = [source("mask16_nearest" if i & 1 else "mask8_nearest", 60 + i, SRC_W, SRC_H) for i in range(len(angles))]
    arena, descs = pack(masks)
    assert sorted({d.elem_bytes for d in descs}) == [1, 2]
    out = A.out_desc(channels=1, channel_major=False, dtype="uint16", item_stride=(131 * 83 * 2 + 15) // 16 * 16 + 16)
    src = torch.from_numpy(arena).to("cuda")
    dst = torch.full((len(masks) * out.item_stride,), 0xAB, dtype=torch.uint8, device="cuda")
    ctx.mask_batch(descs, src.data_ptr(), params, out, dst.data_ptr())
    ctx.synchronize()
    host = dst.cpu().numpy().reshape(len(masks), out.item_stride)
    assert np.all(host[:, 131 * 83 * 2:] == 0xAB)
    for i, (m, p) in enumerate(zip(masks, params)):
        form = "mask16_nearest" if m.dtype == np.uint16 else "mask8_nearest"
        (ref,) = rotate_in_oracle(form, [m], [p])
        got = host[i, :131 * 83 * 2].view(np.uint16).reshape(83, 131, 1)
        assert np.array_equal(got, ref.astype(np.uint16)), (i, form, p.angle)
