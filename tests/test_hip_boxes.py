"""GPU: the box-target kernel (aeon_amd/csrc/box_kernels.hip through aeon_hip_box_targets_batch) against
tests/box_ref.py, bit for bit -- every step on both sides is one correctly rounded float32 operation, so
there is no tolerance.  Windows of 5 and 9 records (a partial last workgroup of four waves); per-record
box counts 0, 1, 63, 64, 65 and 130 (empty records, a full 64-lane chunk, a second and a third chunk);
max_boxes 1, 64 and 70 (truncation after compaction, inside the second chunk); emit none / center /
min_overlap 0.9; flip on and off; expand ratio 1 and 3 with offset (100, 100); a crop that drops every
box; inexact scale quotients (300 / 7, 224 / 171, normalisation by 300); fractional coordinates.  The
output buffers start as 0xCD bytes, so the zero fill of every item is part of the comparison.

Then the decode stage end to end: [localization_ssd, image] and [image, boundingbox] configurations
against box_ref over the params make_ssd_params / make_params give on the same slot engines, with the
image output against the oracle; pixels and boxes against each other without box_ref; the refusals."""
import ctypes

import numpy as np
import pytest

import aeon_amd as A
from aeon_amd import configs as CFG
from tests import box_cases as C
from tests import box_ref as B
from tests import helpers as H
from tests.decoder_cases import (CLASSES, IMG_ETL, SIDE, SSD_AUG, SSD_ETL, as_records, assert_outputs, box_window,
                                 meta_json, ssd_reference)

pytestmark = pytest.mark.gpu

SRC_W, SRC_H = 200, 160
COUNTS = {5: [65, 0, 130, 1, 63], 9: [0, 1, 63, 64, 65, 130, 3, 64, 130]}
EMITS = {"none": (A.EMIT_NONE, 0.0), "center": (A.EMIT_CENTER, 0.0), "min_overlap": (A.EMIT_MIN_OVERLAP, 0.9)}
EXPAND = dict(expand_ratio=3.0, expand_x=100, expand_y=100, expand_w=3 * SRC_W, expand_h=3 * SRC_H)
PLAIN = dict(expand_ratio=1.0, expand_w=SRC_W, expand_h=SRC_H)
PARAMS = [
    dict(PLAIN, crop_x=0, crop_y=0, crop_w=SRC_W, crop_h=SRC_H, out_w=300, out_h=300, flip=0),
    dict(PLAIN, crop_x=13, crop_y=7, crop_w=171, crop_h=150, out_w=224, out_h=224, flip=1),
    dict(EXPAND, crop_x=90, crop_y=80, crop_w=350, crop_h=333, out_w=300, out_h=300, flip=1),
    dict(PLAIN, crop_x=50, crop_y=40, crop_w=7, crop_h=7, out_w=300, out_h=300, flip=1),
    dict(PLAIN, crop_x=1000, crop_y=1000, crop_w=50, crop_h=50, out_w=224, out_h=224, flip=0),  # drops every box
    dict(EXPAND, crop_x=150, crop_y=130, crop_w=171, crop_h=171, out_w=224, out_h=224, flip=0),
    dict(PLAIN, crop_x=20, crop_y=30, crop_w=120, crop_h=90, out_w=300, out_h=224, flip=0),
]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = A.Context(0)
    yield c
    c.close()


def window(n, seed):
    """n records of COUNTS[n] boxes: whole, quarter-pixel and arbitrary fractional coordinates inside
    the SRC_W x SRC_H image, labels and difficult flags, and one of PARAMS per record."""
    rng = np.random.RandomState(seed)
    recs, params = [], []
    for i, cnt in enumerate(COUNTS[n]):
        x0 = rng.uniform(0, SRC_W - 2, cnt)
        y0 = rng.uniform(0, SRC_H - 2, cnt)
        x1 = np.minimum(x0 + rng.uniform(0, 80, cnt), SRC_W - 1)
        y1 = np.minimum(y0 + rng.uniform(0, 80, cnt), SRC_H - 1)
        b = np.stack([x0, y0, x1, y1], 1)
        kind = rng.randint(0, 3, cnt)[:, None]
        b = np.where(kind == 0, np.round(b), np.where(kind == 1, np.round(b * 4) / 4, b)).astype(np.float32)
        recs.append((b, rng.randint(0, 21, cnt).astype(np.int32), rng.randint(0, 2, cnt).astype(np.int32)))
        params.append(A.aug_params(**PARAMS[(i + seed) % len(PARAMS)]))
    return recs, params


@pytest.mark.parametrize("emit", sorted(EMITS))
@pytest.mark.parametrize("max_boxes", [1, 64, 70])
@pytest.mark.parametrize("n", [5, 9])
def test_ssd_targets_equal_reference(ctx, n, max_boxes, emit):
    recs, params = window(n, seed=max_boxes)
    got = A.box_targets(ctx, recs, params, kind=A.BOX_SSD, max_boxes=max_boxes, out_w=300, out_h=300, emit=EMITS[emit])
    kept_total = 0
    for i, ((b, l, d), p) in enumerate(zip(recs, params)):
        want = B.load_ssd(b, l, d, p, max_boxes, 300, 300, EMITS[emit])
        for name in A.SSD_OUTPUTS:
            assert np.array_equal(got[name][i].view(np.uint32), np.asarray(want[name]).view(np.uint32)), \
                (name, i, got[name][i], want[name])
        kept_total += int(want["gt_box_count"])
    assert kept_total > 0  # the window does keep boxes: the comparison is not over zeros alone


@pytest.mark.parametrize("emit", sorted(EMITS))
@pytest.mark.parametrize("max_boxes", [1, 64, 70])
@pytest.mark.parametrize("n", [5, 9])
def test_boundingbox_targets_equal_reference(ctx, n, max_boxes, emit):
    recs, params = window(n, seed=100 + max_boxes)
    got = A.box_targets(ctx, recs, params, kind=A.BOX_BOUNDINGBOX, max_boxes=max_boxes, emit=EMITS[emit])
    assert got.shape == (n, max_boxes * 16)
    for i, ((b, _, _), p) in enumerate(zip(recs, params)):
        want = B.load_boundingbox(b, p, max_boxes, emit=EMITS[emit])
        assert np.array_equal(got[i].view(np.uint32), want.view(np.uint32)), (i, got[i], want)


def test_counts_cover_every_path():
    """What the windows above are meant to reach, shown on the reference: a record that keeps more than
    max_boxes, one that keeps boxes from its second chunk of 64, one that keeps none."""
    for seed in (64, 70, 164, 170):
        recs, params = window(9, seed=seed)
        kept = [B.transform(b, p) for (b, _, _), p in zip(recs, params)]
        assert max(len(k) for k in kept) > 70, seed
        assert any(i >= 64 for k in kept for i, _ in k[:64]), seed  # a second-chunk box inside max_boxes
        dropped_all = [len(k) for k, (r, p) in zip(kept, zip(recs, params)) if p.crop_x == 1000 and len(r[0])]
        assert dropped_all and not any(dropped_all), seed


def test_device_memory_outputs(ctx):
    """The same call into device memory (the decoder's outputs_on_device route), asynchronous on a
    stream, the buffers starting as 0xFF."""
    import torch
    recs, params = window(9, seed=7)
    mb = 64
    sizes = [8, mb * 16, 4, mb * 4, mb * 4]
    bufs = [torch.full((9 * s,), 0xFF, dtype=torch.uint8, device="cuda") for s in sizes]
    stream = torch.cuda.current_stream().cuda_stream
    emit = EMITS["center"]
    assert A.box_targets(ctx, recs, params, kind=A.BOX_SSD, max_boxes=mb, out_w=300, out_h=224, emit=emit,
                         out_ptrs=[t.data_ptr() for t in bufs], stream=stream) is None
    ctx.synchronize(stream)
    host = [t.cpu().numpy() for t in bufs]
    for i, ((b, l, d), p) in enumerate(zip(recs, params)):
        want = B.load_ssd(b, l, d, p, mb, 300, 224, emit)
        for k, name in enumerate(A.SSD_OUTPUTS):
            item = host[k][i * sizes[k]:(i + 1) * sizes[k]].view(np.uint32)
            assert np.array_equal(item, np.ascontiguousarray(want[name]).reshape(-1).view(np.uint32)), (name, i)


@pytest.mark.parametrize("case", C.transform_cases(), ids=lambda c: c[0])
def test_known_answers_through_kernel(ctx, case):
    """aeon's own known answers (tests/box_cases.py) straight through the kernel."""
    _, boxes, params, emit, expect = case
    b = np.asarray(boxes, np.float32)
    rec = (b, np.zeros(len(b), np.int32), np.zeros(len(b), np.int32))
    got = A.box_targets(ctx, [rec], [A.aug_params(**params)], kind=A.BOX_BOUNDINGBOX, max_boxes=16, emit=emit)[0]
    assert [B.rect(got[4 * i:4 * i + 4]) for i in range(len(expect))] == expect
    assert not got[4 * len(expect):].any()


def test_loader_known_answers_through_kernel(ctx):
    """boundingbox.load_pad / load_full and localization_ssd.transform / loader."""
    b = np.asarray(C.GRID_BOXES, np.float32)
    rec = (b, np.zeros(8, np.int32), np.zeros(8, np.int32))
    ident = A.aug_params(**C.identity(256, 256))
    for _, mb in C.LOAD_CASES:
        got = A.box_targets(ctx, [rec], [ident], kind=A.BOX_BOUNDINGBOX, max_boxes=mb)[0]
        k = min(mb, 8)
        assert got[:4 * k].tolist() == b[:k].reshape(-1).tolist() and not got[4 * k:].any()
    t = C.SSD_LOADER
    b = np.asarray(t["boxes"], np.float32)
    got = A.box_targets(ctx, [(b, t["labels"], t["difficult"])], [A.aug_params(**C.identity(100, 100))], kind=A.BOX_SSD,
                        max_boxes=64, out_w=100, out_h=100)
    F = np.float32
    want = [[F(v[0] / F(100)), F(v[1] / F(100)), F(F(v[2] + F(1)) / F(100)), F(F(v[3] + F(1)) / F(100))] for v in b]
    assert got["gt_boxes"][0, :3].tolist() == want and not got["gt_boxes"][0, 3:].any()
    assert got["image_shape"][0].tolist() == [100, 100] and got["gt_box_count"][0] == 3
    assert got["gt_class_count"][0, :4].tolist() == [0, 1, 2, 0] and got["difficult_flag"][0, :4].tolist() == [0, 1, 1, 0]
    s = C.SSD_TRANSFORM
    b = np.asarray(s["boxes"], np.float32)
    got = A.box_targets(ctx, [(b, [0, 0, 0], [0, 0, 0])], [A.aug_params(**s["params"])], kind=A.BOX_BOUNDINGBOX,
                        max_boxes=4)[0]
    want = [[v[0] * 3, v[1] * 3, (v[2] + 1) * 3 - 1, (v[3] + 1) * 3 - 1] for v in s["flipped"]]
    assert got[:12].reshape(3, 4).tolist() == want


def test_box_call_refusals(ctx):
    """Rotation (aeon's transformer returns null there) and boundingbox::box::expand's precondition are
    refused on the host; the context stays usable."""
    rec = (np.array([[10, 10, 50, 50]], np.float32), [0], [0])
    ok = dict(PLAIN, crop_x=0, crop_y=0, crop_w=SRC_W, crop_h=SRC_H, out_w=100, out_h=80)
    with pytest.raises(A.AeonHipError) as e:
        A.box_targets(ctx, [rec], [A.aug_params(**dict(ok, angle=5))], kind=A.BOX_BOUNDINGBOX, max_boxes=4)
    assert e.value.code == A.AEON_HIP_EINVAL and "angle" in str(e.value)
    bad = dict(ok, expand_ratio=2.0, expand_x=80, expand_y=0, expand_w=120, expand_h=320)  # 50 + 80 > 120
    with pytest.raises(A.AeonHipError) as e:
        A.box_targets(ctx, [rec], [A.aug_params(**bad)], kind=A.BOX_BOUNDINGBOX, max_boxes=4)
    assert e.value.code == A.AEON_HIP_EINVAL and "Invalid parameters to expand boundingbox" in str(e.value)
    with pytest.raises(A.AeonHipError):
        A.box_targets(ctx, [rec], [A.aug_params(**ok)], kind=A.BOX_BOUNDINGBOX, max_boxes=0)
    got = A.box_targets(ctx, [rec], [A.aug_params(**ok)], kind=A.BOX_BOUNDINGBOX, max_boxes=4)[0]
    assert got[:4].tolist() == [5.0, 5.0, 24.5, 24.5] and not got[4:].any()


# ---- the decode stage: [localization_ssd, image] and [image, boundingbox] -------------------------------
@pytest.mark.parametrize("lighting", [False, True])
def test_decoder_ssd_then_image_host_outputs(lighting):
    """decode_encoded into pageable host outputs (device staging + D2H), two windows of 12 and 5 records:
    with lighting the second window starts from the cached normal draw the first one left (the
    make_params_split hand-off through make_ssd_params), and its odd size leaves one again."""
    aug = dict(SSD_AUG, lighting=[0.0, 0.1]) if lighting else SSD_AUG
    d = A.Decoder(dict(batch_size=1, random_seed=11, etl=[SSD_ETL, IMG_ETL], augmentation=[aug]))
    f, states = A.ParamFactory(aug), A.seed_slots(11, 12)
    kept = 0
    for window, n in enumerate((12, 5, 12)):
        recs = box_window(n, seed=40 + window)
        want, params = ssd_reference(recs, f, states, aug)
        assert_outputs(d.decode_named(as_records(recs)), want, f"window {window}")
        kept += int(want["gt_box_count"].sum())
    assert kept > 10


def test_decoder_ssd_submit_wait_device_outputs_and_batch_major_false():
    """submit / wait over three windows with different boxes, two in flight, into device outputs; then the
    same windows with batch_major=false (each output transposed per batch, element size 4) into pinned
    host outputs (the zero-copy route)."""
    import torch
    import oracle as O
    cfg = dict(batch_size=4, random_seed=23, etl=[SSD_ETL, IMG_ETL], augmentation=[SSD_AUG])
    d = A.Decoder(cfg)
    f, states = A.ParamFactory(SSD_AUG), A.seed_slots(23, 12)
    windows = [box_window(12, seed=60 + k) for k in range(3)]
    wants = [ssd_reference(w, f, states, SSD_AUG)[0] for w in windows]
    bufs = [[torch.full((12 * o["item_bytes"],), 0xFF, dtype=torch.uint8, device="cuda") for o in d.outputs]
            for _ in range(3)]
    encs = [d.encoded(as_records(w)) for w in windows]
    d.submit(encs[0], [t.data_ptr() for t in bufs[0]], on_device=True)
    d.submit(encs[1], [t.data_ptr() for t in bufs[1]], on_device=True)
    d.wait()
    d.submit(encs[2], [t.data_ptr() for t in bufs[2]], on_device=True)
    d.wait()
    d.wait()
    raw = []
    for k in range(3):
        got = {o["name"]: t.cpu().numpy().view(o["dtype"]) for o, t in zip(d.outputs, bufs[k])}
        assert_outputs(got, wants[k], f"device window {k}")
        raw.append({o["name"]: t.cpu().numpy() for o, t in zip(d.outputs, bufs[k])})
    # batch_major=false, pinned host outputs
    d2 = A.Decoder(dict(cfg, batch_major=False))
    ptrs = []
    try:
        for o in d2.outputs:
            p = ctypes.c_void_p()
            A._check(A.lib().aeon_hip_host_alloc(12 * o["item_bytes"], ctypes.byref(p)))
            ptrs.append(p)
        for k in range(3):
            for p, o in zip(ptrs, d2.outputs):
                ctypes.memset(p, 0xEE, 12 * o["item_bytes"])
            d2.submit(encs[k], [p.value for p in ptrs])
            d2.wait()
            for p, o in zip(ptrs, d2.outputs):
                item = o["item_bytes"]
                got = np.frombuffer(ctypes.string_at(p, 12 * item), np.uint8)
                for b in range(3):
                    blk = raw[k][o["name"]][b * 4 * item:(b + 1) * 4 * item]
                    assert np.array_equal(got[b * 4 * item:(b + 1) * 4 * item], O.transpose(blk, 4, item // 4, 4)), \
                        (k, o["name"], b)
    finally:
        for p in ptrs:
            A.lib().aeon_hip_host_free(p)


def test_pixels_and_boxes_agree():
    """Independent of box_ref: black images with three disjoint boxes, each filled with its own colour;
    flip, expand and patch sampling on, photometric off, emit constraint center (a kept box has its
    centre, so at least half of each side, inside the crop).  The output pixel at the centre of every
    kept gt_box has that box's colour.  Boxes are >= 24 px in a 160 px source, the canvas at most twice
    that and the patch at least half of it, so a kept box spans >= 24 / 2 * 128 / 320 = 4.8 output pixels
    per axis; the test asserts >= 4 through box_ref, and that boxes are kept at all."""
    aug = {"type": "image", "crop_enable": False, "flip_enable": True, "expand_ratio": [1.0, 2.0],
           "expand_probability": 0.5, "emit_constraint_type": "center",
           "batch_samplers": [{"max_sample": 1, "max_trials": 50, "sampler": {"scale": [0.5, 1.0]}}]}
    ssd = dict(SSD_ETL, max_gt_boxes=8)
    img_etl = {"type": "image", "height": SIDE, "width": SIDE, "channels": 3, "output_type": "uint8_t",
               "channel_major": False}
    colours = [(255, 40, 40), (40, 255, 40), (40, 40, 255)]
    rng = np.random.default_rng(5)
    recs = []
    for i in range(16):
        img = np.zeros((160, 160, 3), np.uint8)
        boxes = []
        for j, x_lo in enumerate((2, 56, 110)):  # one box per vertical band: disjoint
            bw, bh = int(rng.integers(24, 48)), int(rng.integers(24, 100))
            x0, y0 = x_lo + int(rng.integers(0, 48 - bw + 1)), int(rng.integers(0, 160 - bh))
            boxes.append((float(x0), float(y0), float(x0 + bw - 1), float(y0 + bh - 1)))
            img[y0:y0 + bh, x0:x0 + bw] = colours[j]
        recs.append(dict(img=img, w=160, h=160, boxes=boxes, labels=[0, 1, 2], difficult=[0, 0, 0]))
    d = A.Decoder(dict(batch_size=16, random_seed=3, etl=[ssd, img_etl], augmentation=[aug]))
    out = d.decode_named(as_records(recs))
    f, states = A.ParamFactory(aug), A.seed_slots(3, 16)
    checked = 0
    for i, r in enumerate(recs):
        p = f.make_ssd_params(states[i:i + 1], 160, 160, SIDE, SIDE, r["boxes"])
        kept = B.transform(r["boxes"], p, *f.emit())
        assert out["gt_box_count"][i].item() == len(kept)
        for slot, (_, t) in enumerate(kept):
            assert t[2] - t[0] + 1 >= 4 and t[3] - t[1] + 1 >= 4, (i, slot, t)
            x0, y0, x1, y1 = (float(v) * SIDE for v in out["gt_boxes"][i, slot])
            cx, cy = int((x0 + x1) / 2), int((y0 + y1) / 2)  # x1 = xmax + 1: the middle pixel
            label = int(out["gt_class_count"][i, slot, 0])
            assert tuple(out["image"][i, cy, cx]) == colours[label], (i, slot, cx, cy, out["image"][i, cy, cx])
            checked += 1
    assert checked >= 12


def test_decoder_image_then_boundingbox():
    """[image, boundingbox]: the image draws (make_params cropping: scale [0.6, 0.8], flip), the
    boundingbox provider reuses its params."""
    aug = {"type": "image", "scale": [0.6, 0.8], "center": False, "flip_enable": True,
           "emit_constraint_type": "min_overlap", "emit_constraint_min_overlap": 0.3}
    bb = {"type": "boundingbox", "height": 96, "width": 96, "max_bbox_count": 3, "class_names": CLASSES}
    img_etl = dict(IMG_ETL, height=96, width=96)
    d = A.Decoder(dict(batch_size=7, random_seed=17, etl=[img_etl, bb], augmentation=[aug]))
    recs = box_window(7, seed=80)
    f, states = A.ParamFactory(aug), A.seed_slots(17, 7)
    params = [f.make_params(states[i:i + 1], r["w"], r["h"], 96, 96) for i, r in enumerate(recs)]
    out = d.decode_named([(r["img"], meta_json(r["w"], r["h"], r["boxes"], r["labels"], r["difficult"])) for r in recs])
    want = np.stack([B.load_boundingbox(r["boxes"], p, 3, emit=f.emit()) for r, p in zip(recs, params)])
    assert out["boundingbox"].shape == (7, 3, 16)
    assert np.array_equal(out["boundingbox"].reshape(7, -1).view(np.uint32), want.view(np.uint32))
    assert want.any()
    ref = np.stack(H.oracle_records([r["img"] for r in recs], params, CFG.out_desc_for(img_etl, aug)))
    assert np.array_equal(out["image"], ref)


def test_decoder_refuses_rotation_and_stays_usable():
    """angle in {0, 1}: a window (one record each) whose record drew a non-zero angle fails with
    AEON_HIP_EINVAL (aeon's transformer returns a null pointer there); the windows after it still
    decode, with the engines where aeon's would be."""
    aug = {"type": "image", "crop_enable": False, "angle": [0, 1]}
    d = A.Decoder(dict(batch_size=1, random_seed=29, etl=[SSD_ETL, IMG_ETL], augmentation=[aug]))
    f, states = A.ParamFactory(aug), A.seed_slots(29, 1)
    seen = set()
    for k in range(10):
        recs = box_window(1, seed=90 + k)
        want, params = ssd_reference(recs, f, states, aug)
        if params[0].angle != 0:
            with pytest.raises(A.AeonHipError) as e:
                d.decode_named(as_records(recs))
            assert e.value.code == A.AEON_HIP_EINVAL and "angle" in str(e.value)
        else:
            assert_outputs(d.decode_named(as_records(recs)), want, f"window {k}")
        seen.add(params[0].angle != 0)
    assert seen == {True, False}


def test_decoder_empty_metadata_message():
    d = A.Decoder(dict(batch_size=2, random_seed=31, etl=[SSD_ETL, IMG_ETL], augmentation=[SSD_AUG]))
    recs = box_window(2, seed=99)
    bad = as_records(recs)
    bad[1] = (b"", bad[1][1])
    with pytest.raises(A.AeonHipError) as e:
        d.decode_named(bad)
    assert "received localization_ssd data with size 0, at idx 1" in str(e.value)
    # the failed window drew nothing: the next one gets the first window's engines
    f, states = A.ParamFactory(SSD_AUG), A.seed_slots(31, 2)
    want, _ = ssd_reference(recs, f, states, SSD_AUG)
    assert_outputs(d.decode_named(as_records(recs)), want, "after the failure")
    bb = {"type": "boundingbox", "height": 96, "width": 96, "max_bbox_count": 3, "class_names": CLASSES}
    d = A.Decoder(dict(batch_size=1, etl=[IMG_ETL, bb], augmentation=[SSD_AUG]))
    with pytest.raises(A.AeonHipError) as e:
        d.decode_named([(recs[0]["img"], b"")])
    assert "received boundingbox with size 0, at idx 0" in str(e.value)
