"""GPU: the localization_rcnn targets kernel (aeon_amd/csrc/rcnn_kernels.hip through
aeon_hip_rcnn_targets_batch and the decoder) against tests/rcnn_ref.py.

Everything is compared as uint32 bit patterns with no tolerance, except dw and dh (planes 2 and 3 of
bbtargets): those may differ from rcnn_ref's value -- the float64 log of the float32 quotient, rounded --
by at most 2 float32 ulps, since HIP documents logf at 1 ulp and glibc's is within 1 ulp.  The output
buffers start as 0xCD bytes, so the fills of every item are part of the comparison.

Small anchor grids (base_size 16, scales 1 2 3, ratios 0.5 1 2, scaling_factor 1/16): 80 x 48 (135
anchors: under one workgroup stride, not a multiple of 64, and odd, so the second record's labels_flat
item is not 16-byte aligned) and 400 x 304 (4275: several strides); windows of 1, 5 and 9 records; 0, 1, 6,
64, 65 and 130 boxes per record (none, over max_gt_boxes, over a wave's 64 and twice that); shuffle off and
on; a crop that drops some boxes and one that drops all, a flip, and a cropbox that scales to an image
smaller than the grid (anchors outside).  Named cases are asserted on the reference before the comparison.
Then aeon's own known answer at its shape (34 596 anchors), a 1200 x 1200 grid whose background list is
longer than 46 340 (std::shuffle's other form), and the decode stage end to end."""
import ctypes
import json
import os

import numpy as np
import pytest

import aeon_amd as A
from aeon_amd import configs as CFG
from tests import box_cases as C
from tests import box_ref as B
from tests import helpers as H
from tests import rcnn_ref as R
from tests.decoder_cases import (CLASSES, IMG_ETL, SIDE, SSD_AUG, SSD_ETL, as_records, assert_outputs, box_window,
                                 ssd_reference)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "rcnn_kat.json")))
BASE = dict(type="localization_rcnn", class_names=CLASSES, base_size=16, scales=[1, 2, 3], ratios=[0.5, 1, 2],
            scaling_factor=1.0 / 16.0)
GRIDS = {"80x48": (80, 48), "400x304": (400, 304)}
COUNTS = {1: [6], 5: [65, 0, 130, 1, 6], 9: [0, 1, 6, 64, 65, 130, 6, 64, 130]}
F = np.float32


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = A.Context(0)
    yield c
    c.close()


def grid_cfg(grid, **kw):
    w, h = GRIDS[grid]
    return dict(BASE, width=w, height=h, **kw)


def params_for(w, h, fixed_scaling_factor=-1.0):
    """The params the windows cycle through; output_size = round(cropbox * scale), as make_params sets it."""
    crops = [dict(crop_x=0, crop_y=0, crop_w=w, crop_h=h, flip=0),
             dict(crop_x=13, crop_y=7, crop_w=w - 40, crop_h=h - 20, flip=1),       # drops some boxes, flips
             dict(crop_x=w // 4, crop_y=h // 4, crop_w=w // 2, crop_h=h // 4, flip=0),  # scales to w x h/2
             dict(crop_x=10 * w, crop_y=10 * h, crop_w=50, crop_h=50, flip=0),       # drops every box
             dict(crop_x=5, crop_y=3, crop_w=w - 9, crop_h=h - 5, flip=1)]
    out = []
    for c in crops:
        s = F(fixed_scaling_factor) if fixed_scaling_factor > 0 else F(A.calculate_scale(c["crop_w"], c["crop_h"], w, h))
        out.append(A.aug_params(expand_ratio=1.0, expand_w=w, expand_h=h,
                                out_w=A.unbiased_round(float(F(F(c["crop_w"]) * s))),
                                out_h=A.unbiased_round(float(F(F(c["crop_h"]) * s))), **c))
    return out


def window(grid, n, seed):
    """n records of COUNTS[n] boxes (whole, quarter-pixel and arbitrary coordinates) inside the grid's image."""
    w, h = GRIDS[grid]
    rng = np.random.RandomState(seed)
    plist = params_for(w, h)
    recs, params = [], []
    for i, cnt in enumerate(COUNTS[n]):
        x0, y0 = rng.uniform(0, w - 2, cnt), rng.uniform(0, h - 2, cnt)
        x1 = np.minimum(x0 + rng.uniform(0, w / 2, cnt), w - 1)
        y1 = np.minimum(y0 + rng.uniform(0, h / 2, cnt), h - 1)
        b = np.stack([x0, y0, x1, y1], 1)
        kind = rng.randint(0, 3, cnt)[:, None]
        b = np.where(kind == 0, np.round(b), np.where(kind == 1, np.round(b * 4) / 4, b)).astype(np.float32)
        recs.append((b, rng.randint(0, 3, cnt).astype(np.int32), rng.randint(0, 2, cnt).astype(np.int32)))
        params.append(plist[(i + seed) % len(plist)])
    return recs, params


def reference(cfg, recs, params, states, shuffle, **kw):
    """rcnn_ref over the records, the engine states advanced in place: [(outputs, transform, sampled)]."""
    anchors, info = A.rcnn_anchors(cfg), A.rcnn_config_info(cfg)
    return [R.record(cfg, anchors, r, p, state=states[i:i + 1], shuffle=shuffle, info=info, **kw)
            for i, (r, p) in enumerate(zip(recs, params))]


def compare(got, want, states_got, states_want, what):
    for i, (w, _, _) in enumerate(want):
        R.assert_equal({k: got[k][i] for k in A.RCNN_OUTPUTS}, w, (what, i))
    assert np.array_equal(states_got, states_want), what


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("n", [1, 5, 9])
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_small_grids_equal_reference(ctx, grid, n, shuffle):
    cfg = grid_cfg(grid)
    recs, params = window(grid, n, seed=n)
    s_ref = A.seed_slots(7 + n, n)
    s_gpu = s_ref.copy()
    want = reference(cfg, recs, params, s_ref, shuffle)
    got = A.rcnn_targets(ctx, cfg, recs, params, states=s_gpu, shuffle=shuffle)
    compare(got, want, s_gpu, s_ref, (grid, n, shuffle))
    sampled = sum(len(s) for _, _, s in want)
    assert sampled > 0 and (not shuffle or not np.array_equal(s_ref, A.seed_slots(7 + n, n)))


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_gt_counts_around_the_tiles(ctx, grid):
    """Whole-image params keep every box: K is exactly 0, 1, 6, 64, 65 and 130 (none, max_gt_boxes, one over
    it and over a wave's 64 lanes, two over twice that)."""
    cfg = grid_cfg(grid)
    w, h = GRIDS[grid]
    recs = [r for n in (5, 9) for r in window(grid, n, seed=n)[0]]
    recs = [next(r for r in recs if len(r[0]) == k) for k in (0, 1, 6, 64, 65, 130)]
    params = [params_for(w, h)[0]] * len(recs)
    s_ref, s_gpu = A.seed_slots(21, len(recs)), A.seed_slots(21, len(recs))
    want = reference(cfg, recs, params, s_ref, True)
    assert [len(t["gt"]) for _, t, _ in want] == [0, 1, 6, 64, 65, 130]
    assert [o["gt_box_count"].item() for o, _, _ in want] == [0, 1, 6, 64, 64, 64]
    got = A.rcnn_targets(ctx, cfg, recs, params, states=s_gpu, shuffle=True)
    compare(got, want, s_gpu, s_ref, ("counts", grid))


def test_windows_cover_the_paths():
    """What the windows above reach, shown on the reference: records keeping more than max_gt_boxes, more
    than 64 and more than 128 boxes, a crop that drops every box and one that drops some, anchors outside
    the image, a gt box that overlaps no inside anchor (every inside anchor foreground, no background),
    more foreground than num_fg, fewer background anchors than the remainder (80 x 48) and fewer foreground
    than num_fg with background taking the remainder (400 x 304)."""
    ks, all_fg = [], False
    for grid in sorted(GRIDS):
        cfg = grid_cfg(grid)
        info = A.rcnn_config_info(cfg)
        fewer_bg = fewer_fg = more_fg = False
        for n in (5, 9):
            recs, params = window(grid, n, seed=n)
            want = reference(cfg, recs, params, A.seed_slots(1, n), False)
            ks += [(len(r[0]), len(t["gt"])) for r, (_, t, _) in zip(recs, want)]
            assert any(0 < len(t["idx_inside"]) < len(t["labels"]) // 2 for _, t, _ in want)
            for _, t, s in want:
                n_fg, n_bg = int((t["labels"] == 1).sum()), int((t["labels"] == 0).sum())
                take_fg = min(n_fg, info["num_fg"])
                assert len(s) == take_fg + min(n_bg, info["rois_per_image"] - take_fg)
                fewer_bg |= 0 < n_bg < info["rois_per_image"] - take_fg
                fewer_fg |= 0 < n_fg < info["num_fg"] and n_bg >= info["rois_per_image"] - n_fg
                more_fg |= n_fg > info["num_fg"]
                all_fg |= len(t["gt"]) > 0 and not t["overlaps"].any(axis=0).all() and n_fg == len(t["idx_inside"]) > 0
        assert (fewer_bg if grid == "80x48" else fewer_fg and more_fg), grid
    assert all_fg
    assert any(k > 128 for _, k in ks) and any(64 < k <= 128 for _, k in ks)
    assert any(c > 0 and k == 0 for c, k in ks) and any(0 < k < c for c, k in ks)


def one_record(boxes):
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    return (b, np.arange(len(b), dtype=np.int32) % 3, np.zeros(len(b), np.int32))


@pytest.mark.parametrize("shuffle", [False, True])
def test_gt_box_overlapping_no_inside_anchor_and_more_foreground_than_num_fg(ctx, shuffle):
    """The image is half the grid (fixed_scaling_factor 0.5 over a full crop) while the boxes keep their
    place (output_size = cropbox): the second box lies outside the scaled image, overlaps no inside anchor,
    has column maximum 0 -- and aeon makes every inside anchor foreground.  With rois_per_image 16 that is
    more foreground than num_fg = 8, and no background at all."""
    cfg = grid_cfg("400x304", rois_per_image=16)
    p = A.aug_params(crop_x=0, crop_y=0, crop_w=400, crop_h=304, out_w=400, out_h=304, flip=0, expand_ratio=1.0)
    rec = one_record([[20, 20, 60, 70], [300, 200, 380, 290]])
    s_ref, s_gpu = np.array([12345], np.uint32), np.array([12345], np.uint32)
    want = reference(cfg, [rec], [p], s_ref, shuffle, fixed_scaling_factor=0.5)
    _, t, sampled = want[0]
    assert (t["im_w"], t["im_h"]) == (200, 152) and not t["overlaps"][:, 1].any() and t["overlaps"][:, 0].any()
    assert len(t["idx_inside"]) > 100 and (t["labels"][t["idx_inside"]] == 1).all()
    assert len(sampled) == 8  # num_fg foreground, nothing to fill the remainder with
    got = A.rcnn_targets(ctx, cfg, [rec], [p], states=s_gpu, shuffle=shuffle, fixed_scaling_factor=0.5)
    compare(got, want, s_gpu, s_ref, "no-overlap gt box")


def test_tie_on_a_column_maximum_and_overlap_equal_to_threshold(ctx):
    """Two 16 x 16 anchors overlap the box (0, 8, 15, 23) by exactly 1/3 each, the column's maximum: both
    are foreground.  With positive_overlap 0.5, an anchor holding exactly half of the box (4, 0, 35, 15)
    -- not that box's best anchor -- is foreground through `>=` alone."""
    cfg = grid_cfg("80x48", positive_overlap=0.5)
    p = A.aug_params(crop_x=0, crop_y=0, crop_w=80, crop_h=48, out_w=80, out_h=48, flip=0, expand_ratio=1.0)
    recs = [one_record([[0, 8, 15, 23]]), one_record([[4, 0, 35, 15]])]
    s_ref, s_gpu = A.seed_slots(3, 2), A.seed_slots(3, 2)
    want = reference(cfg, recs, [p, p], s_ref, True)
    ov = want[0][1]["overlaps"][:, 0]
    assert (ov == ov.max()).sum() == 2 and ov.max() == F(1) / F(3)
    assert (want[0][1]["labels"][want[0][1]["idx_inside"]][ov == ov.max()] == 1).all()
    t = want[1][1]
    ov = t["overlaps"][:, 0]
    half = np.flatnonzero(ov == F(0.5))
    assert len(half) == 1 and ov.max() > F(0.5) and t["labels"][t["idx_inside"][half[0]]] == 1
    strict = R.transform(dict(A.rcnn_config_info(cfg), positive_overlap=float(np.nextafter(F(0.5), F(1)))),
                         A.rcnn_anchors(cfg), recs[1][0], p)
    assert strict["labels"][t["idx_inside"][half[0]]] == -1  # neither background nor foreground without `>=`
    got = A.rcnn_targets(ctx, cfg, recs, [p, p], states=s_gpu, shuffle=True)
    compare(got, want, s_gpu, s_ref, "tie / threshold")


AEON_CFG = {"type": "localization_rcnn", "height": 1000, "width": 1000, "class_names": C.LABEL_LIST, "max_gt_boxes": 64}
AEON_AUG = {"type": "image", "flip_enable": False, "crop_enable": False, "fixed_aspect_ratio": True,
            "fixed_scaling_factor": 1.6}


def test_aeon_known_answer(ctx):
    """aeon's loader test through the kernel, against aeon's numbers directly (shuffle off), then with the
    shuffle on against rcnn_ref."""
    meta = A.box_extract(C.LABEL_LIST, open(os.path.join(ROOT, "tests", "golden", "voc", "006637.json"), "rb").read())
    p = A.ParamFactory(AEON_AUG).make_params(np.array([1], np.uint32), meta["width"], meta["height"], 1000, 1000)
    got = A.rcnn_targets(ctx, AEON_CFG, [meta], [p], shuffle=False, fixed_scaling_factor=1.6)
    L, A_ = KAT["loader"], KAT["total_anchors"]
    fg = np.array(L["fg_idx"])
    assert np.flatnonzero(got["labels_mask"][0]).tolist() == sorted(L["labels_mask_idx"])
    assert set(got["labels_mask"][0].reshape(-1).tolist()) == {0, 1}
    want_flat = np.concatenate([np.ones(A_, np.int32), np.zeros(A_, np.int32)])
    want_flat[fg], want_flat[fg + A_] = 0, 1
    assert np.array_equal(got["labels_flat"][0].reshape(-1), want_flat)
    want_mask = np.zeros(4 * A_, np.float32)
    want_mask[L["bbox_mask_index"]] = 1
    assert np.array_equal(got["bbtargets_mask"][0].view(np.uint32), want_mask.view(np.uint32))
    want_t = np.zeros(4 * A_, np.float64)
    for i, v in L["bbox_targets"]:
        want_t[i] = v
    assert np.abs(got["bbtargets"][0].astype(np.float64) - want_t).max() <= L["tolerance"]
    assert np.array_equal(got["bbtargets"][0] == 0, want_t == 0)
    assert got["image_shape"][0].reshape(-1).tolist() == L["image_shape"] and got["gt_box_count"][0].item() == 6
    assert got["image_scale"][0].item() == F(1.6)
    anchors = A.rcnn_anchors(AEON_CFG)
    rec = (meta["boxes"], meta["labels"], meta["difficult"])
    want, _, _ = R.record(AEON_CFG, anchors, rec, p, shuffle=False, fixed_scaling_factor=1.6)
    R.assert_equal({k: got[k][0] for k in A.RCNN_OUTPUTS}, want, "shuffle off")
    s_ref, s_gpu = np.array([2024], np.uint32), np.array([2024], np.uint32)
    want, _, sampled = R.record(AEON_CFG, anchors, rec, p, state=s_ref, shuffle=True, fixed_scaling_factor=1.6)
    assert len(sampled) == 256 and sampled.tolist() != L["fg_idx"] + L["bg_idx"]
    got = A.rcnn_targets(ctx, AEON_CFG, [meta], [p], states=s_gpu, shuffle=True, fixed_scaling_factor=1.6)
    R.assert_equal({k: got[k][0] for k in A.RCNN_OUTPUTS}, want, "shuffle on")
    assert s_gpu[0] == s_ref[0]


def test_large_grid_past_the_shuffles_form_switch(ctx):
    """1200 x 1200 with small anchors: 50 625 anchors, and one small box leaves more than 46 340 of them
    background, so the background shuffle draws once per swap (libstdc++'s form above sqrt(2^31))."""
    cfg = dict(BASE, width=1200, height=1200)
    p = A.aug_params(crop_x=0, crop_y=0, crop_w=1200, crop_h=1200, out_w=1200, out_h=1200, flip=0, expand_ratio=1.0)
    rec = one_record([[500, 520, 531, 560]])
    s_ref, s_gpu = np.array([99], np.uint32), np.array([99], np.uint32)
    want = reference(cfg, [rec], [p], s_ref, True)
    _, t, sampled = want[0]
    assert len(t["labels"]) == 50625 and (t["labels"] == 0).sum() > 46340 and 0 < (t["labels"] == 1).sum() < 128
    assert len(sampled) == 256
    got = A.rcnn_targets(ctx, cfg, [rec], [p], states=s_gpu, shuffle=True)
    compare(got, want, s_gpu, s_ref, "large grid")


def test_engine_words_congruent_to_zero_run_as_one(ctx):
    """An engine word of 0, 2^31 - 1 or 2^32 - 2 is what minstd_rand0::seed turns into 1 (taken as it stands,
    the LCG would stay at 0 and every draw be refused): such records sample what a record with state 1
    samples, on the host and on the device, and their engines end where its engine ends."""
    cfg = grid_cfg("400x304")
    recs, params = window("400x304", 1, seed=1)
    recs, params = recs * 4, params * 4
    s_ref = np.array([1, 0, 0x7FFFFFFF, 0xFFFFFFFE], np.uint32)
    s_gpu = s_ref.copy()
    want = reference(cfg, recs, params, s_ref, True)
    assert len(set(s_ref.tolist())) == 1 and s_ref[0] not in (0, 1) and len(want[0][2]) == 256
    assert all(w[2].tolist() == want[0][2].tolist() for w in want)
    got = A.rcnn_targets(ctx, cfg, recs, params, states=s_gpu, shuffle=True)
    compare(got, want, s_gpu, s_ref, "engine words")
    s_gpu = np.array([0], np.uint32)  # no box, no draw: the word comes back as the engine holds it
    A.rcnn_targets(ctx, cfg, [one_record(np.zeros((0, 4)))], params[:1], states=s_gpu, shuffle=True)
    assert s_gpu[0] == 1


def test_direct_call_refusals(ctx):
    cfg = grid_cfg("80x48")
    ok = dict(crop_x=0, crop_y=0, crop_w=80, crop_h=48, out_w=80, out_h=48, flip=0, expand_ratio=1.0)
    rec = one_record([[10, 10, 50, 40]])
    with pytest.raises(A.AeonHipError) as e:
        A.rcnn_targets(ctx, cfg, [rec], [A.aug_params(**dict(ok, angle=5))], shuffle=False)
    assert e.value.code == A.AEON_HIP_EINVAL and "angle" in str(e.value)
    with pytest.raises(A.AeonHipError) as e:  # 9 * 94 * 94 anchors
        A.rcnn_targets(ctx, dict(BASE, scales=[8, 16, 32], width=1504, height=1504), [rec], [A.aug_params(**ok)],
                       shuffle=False)
    assert e.value.code == A.AEON_HIP_EUNSUPPORTED and "total_anchors" in str(e.value)
    with pytest.raises(A.AeonHipError) as e:
        A.rcnn_targets(ctx, dict(cfg, rois_per_image=2000), [rec], [A.aug_params(**ok)], shuffle=False)
    assert e.value.code == A.AEON_HIP_EUNSUPPORTED
    with pytest.raises(A.AeonHipError) as e:
        A.rcnn_targets(ctx, cfg, [one_record(np.tile([[1, 1, 9, 9]], (1025, 1)))], [A.aug_params(**ok)], shuffle=False)
    assert e.value.code == A.AEON_HIP_EUNSUPPORTED
    with pytest.raises(A.AeonHipError) as e:
        A.rcnn_targets(ctx, cfg, [rec], [A.aug_params(**ok)], shuffle=True)  # no engine states
    assert e.value.code == A.AEON_HIP_EINVAL
    got = A.rcnn_targets(ctx, cfg, [rec], [A.aug_params(**ok)], shuffle=False)  # the context stays usable
    assert got["gt_box_count"][0].item() == 1 and got["gt_boxes"][0, 0].tolist() == [10, 10, 50, 40]


# ---- the decode stage: [localization_rcnn, image] ---------------------------------------------------------
RCNN_ETL = dict(BASE, width=SIDE, height=SIDE, max_gt_boxes=4, rois_per_image=32)
RCNN_AUG = {"type": "image", "scale": [0.6, 0.8], "center": False, "flip_enable": True}


def rcnn_reference(recs, f, states, aug, etl=RCNN_ETL):
    """The ten outputs (rcnn_ref over make_params on the slot engines, then the shuffles on the same
    engines, which stay advanced for the next window -- aeon's deterministic mode) and the oracle's image
    records for the same params."""
    anchors, info = A.rcnn_anchors(etl), A.rcnn_config_info(etl)
    outs, params = [], []
    for i, r in enumerate(recs):
        p = f.make_params(states[i:i + 1], r["w"], r["h"], etl["width"], etl["height"])
        o, _, _ = R.record(etl, anchors, (np.asarray(r["boxes"], np.float32).reshape(-1, 4), r["labels"], r["difficult"]),
                           p, state=states[i:i + 1], shuffle=True, emit=f.emit(), info=info,
                           fixed_scaling_factor=aug.get("fixed_scaling_factor", -1.0))
        outs.append(o), params.append(p)
    want = {k: np.stack([o[k] for o in outs]) for k in A.RCNN_OUTPUTS}
    want["image"] = np.stack(H.oracle_records([r["img"] for r in recs], params, CFG.out_desc_for(IMG_ETL, aug)))
    return want, params


def assert_rcnn_outputs(got, want, what):
    for i in range(len(want["bbtargets"])):
        R.assert_equal({k: np.asarray(got[k])[i] for k in A.RCNN_OUTPUTS}, {k: want[k][i] for k in A.RCNN_OUTPUTS},
                       (what, i))
    assert np.array_equal(np.asarray(got["image"]).reshape(want["image"].shape), want["image"]), (what, "image")


def pinned_outputs(d, n, fill):
    ptrs = []
    for o in d.outputs:
        p = ctypes.c_void_p()
        A._check(A.lib().aeon_hip_host_alloc(n * o["item_bytes"], ctypes.byref(p)))
        ctypes.memset(p, fill, n * o["item_bytes"])
        ptrs.append(p)
    return ptrs


def read_outputs(d, ptrs, n):
    return {o["name"]: np.frombuffer(ctypes.string_at(p, n * o["item_bytes"]), np.uint8).view(o["dtype"])
            .reshape((n,) + o["shape"]).copy() for o, p in zip(d.outputs, ptrs)}


@pytest.mark.parametrize("batch_major", [True, False])
def test_decoder_threads_engine_states_through_windows(batch_major):
    """Two windows of 5 records through submit / wait (both in flight), then a third through decode into
    pageable host outputs: every window's shuffles start from the engines the window before left, which the
    reference threads the same way -- a wrong hand-back shows in the second window's sampled anchors."""
    import oracle as O
    cfg = dict(batch_size=5, random_seed=41, etl=[RCNN_ETL, IMG_ETL], augmentation=[RCNN_AUG], batch_major=batch_major)
    d = A.Decoder(cfg)
    f, states = A.ParamFactory(RCNN_AUG), A.seed_slots(41, 5)
    windows = [box_window(5, seed=70 + k) for k in range(3)]
    before = states.copy()
    wants = [rcnn_reference(w, f, states, RCNN_AUG)[0] for w in windows]
    assert not np.array_equal(before, states) and sum(int(w["labels_mask"].sum()) for w in wants) > 100
    encs = [d.encoded(as_records(w)) for w in windows]
    bufs = [pinned_outputs(d, 5, 0xCD) for _ in range(2)]
    try:
        d.submit(encs[0], [p.value for p in bufs[0]])
        d.submit(encs[1], [p.value for p in bufs[1]])
        d.wait()
        d.wait()
        gots = [read_outputs(d, bufs[k], 5) for k in range(2)]
    finally:
        for p in bufs[0] + bufs[1]:
            A.lib().aeon_hip_host_free(p)
    gots.append(d.decode_named(as_records(windows[2])))
    for k, (got, want) in enumerate(zip(gots, wants)):
        if not batch_major:  # each output transposed per batch (one batch of 5 per window), element size 4
            got = {o["name"]: O.transpose(np.ascontiguousarray(got[o["name"]]).reshape(-1).view(np.uint8),
                                          o["item_bytes"] // 4, 5, 4).view(o["dtype"]).reshape((5,) + o["shape"])
                   for o in d.outputs}
        assert_rcnn_outputs(got, want, f"window {k} batch_major={batch_major}")
    d.close()


def test_decoder_rcnn_and_boundingbox_tables_in_one_window():
    """[localization_rcnn, boundingbox, image]: two box tables in one window at different arena offsets,
    the first with the rcnn extension and its padding behind it.  The boundingbox element reuses the params
    the rcnn element drew; the rcnn outputs and the image are the [localization_rcnn, image] reference's."""
    bb = {"type": "boundingbox", "height": SIDE, "width": SIDE, "max_bbox_count": 4, "class_names": CLASSES}
    d = A.Decoder(dict(batch_size=5, random_seed=43, etl=[RCNN_ETL, bb, IMG_ETL], augmentation=[RCNN_AUG]))
    f, states = A.ParamFactory(RCNN_AUG), A.seed_slots(43, 5)
    recs = box_window(5, seed=85)
    want, params = rcnn_reference(recs, f, states, RCNN_AUG)
    got = d.decode_named([(meta, meta, img) for meta, img in as_records(recs)])
    d.close()
    assert_rcnn_outputs(got, want, "rcnn + boundingbox")
    want_bb = np.stack([B.load_boundingbox(r["boxes"], p, 4, emit=f.emit()) for r, p in zip(recs, params)])
    assert got["boundingbox"].shape == (5, 4, 16)
    assert np.array_equal(got["boundingbox"].reshape(5, -1).view(np.uint32), want_bb.view(np.uint32))
    assert want_bb.any() and sum(len(r["boxes"]) for r in recs) % 2 == 1  # the extension follows 8 bytes of padding


def test_decoder_seed_zero_invariants():
    """random_seed 0: the draws are not reproducible, so with an augmentation that draws nothing that
    matters (no crop, no flip) the labels are known and the sample is checked for what must hold: its
    size, sampled anchors among the labelled ones, foreground capped at num_fg, targets only there."""
    aug = {"type": "image", "crop_enable": False, "flip_enable": False}
    d = A.Decoder(dict(batch_size=4, etl=[RCNN_ETL, IMG_ETL], augmentation=[aug]))
    recs = box_window(4, seed=77)
    got = d.decode_named(as_records(recs))
    f = A.ParamFactory(aug)
    anchors, info = A.rcnn_anchors(RCNN_ETL), A.rcnn_config_info(RCNN_ETL)
    A_ = len(anchors)
    seen = 0
    for i, r in enumerate(recs):
        p = f.make_params(np.array([1], np.uint32), r["w"], r["h"], SIDE, SIDE)
        t = R.transform(info, anchors, r["boxes"], p, f.emit())
        lm, lf = got["labels_mask"][i].reshape(-1), got["labels_flat"][i].reshape(-1)
        sel = np.flatnonzero(lm[:A_])
        assert np.array_equal(lm[:A_], lm[A_:]) and (t["labels"][sel] >= 0).all()
        fg = sel[t["labels"][sel] == 1]
        n_fg, n_bg = int((t["labels"] == 1).sum()), int((t["labels"] == 0).sum())
        take_fg = min(n_fg, info["num_fg"])
        assert len(fg) == take_fg and len(sel) == take_fg + min(n_bg, info["rois_per_image"] - take_fg)
        assert np.array_equal(np.flatnonzero(lf[A_:]), fg) and np.array_equal(lf[:A_], 1 - lf[A_:])
        assert np.array_equal(np.flatnonzero(got["bbtargets_mask"][i][:A_]), fg)
        assert set(np.flatnonzero(got["bbtargets"][i]) % A_) <= set(sel.tolist())
        assert got["gt_box_count"][i].item() == min(4, len(t["gt"]))
        seen += len(sel)
    assert seen > 0
    d.close()


def test_decoder_refusals():
    aug = {"type": "image", "crop_enable": False, "angle": [5, 5]}
    d = A.Decoder(dict(batch_size=1, random_seed=5, etl=[RCNN_ETL, IMG_ETL], augmentation=[aug]))
    with pytest.raises(A.AeonHipError) as e:
        d.decode_named(as_records(box_window(1, seed=3)))
    assert e.value.code == A.AEON_HIP_EINVAL and "angle" in str(e.value)
    d.close()
    with pytest.raises(A.AeonHipError) as e:  # 9 * 94 * 94 anchors: above the stated 65 536
        A.Decoder(dict(batch_size=1, etl=[dict(BASE, scales=[8, 16, 32], width=1504, height=1504), IMG_ETL]))
    assert e.value.code == A.AEON_HIP_EUNSUPPORTED
    d = A.Decoder(dict(batch_size=1, random_seed=5, etl=[RCNN_ETL, IMG_ETL], augmentation=[RCNN_AUG]))
    recs = as_records(box_window(1, seed=3))
    with pytest.raises(A.AeonHipError) as e:
        d.decode_named([(b"", recs[0][1])])
    assert "received localization_rcnn data with size 0, at idx 0" in str(e.value)
    d.close()


def test_other_configurations_are_unchanged():
    """An [image]-only and a [localization_ssd, image] configuration give what they gave before: the
    oracle's pixels and box_ref's boxes, over two windows each."""
    aug = {"type": "image", "scale": [0.6, 0.8], "center": False, "flip_enable": True}
    d = A.Decoder(dict(batch_size=6, random_seed=13, etl=[IMG_ETL], augmentation=[aug]))
    f, states = A.ParamFactory(aug), A.seed_slots(13, 6)
    for k in range(2):
        recs = box_window(6, seed=50 + k)
        params = [f.make_params(states[i:i + 1], r["w"], r["h"], IMG_ETL["width"], IMG_ETL["height"]) for i, r in enumerate(recs)]
        ref = np.stack(H.oracle_records([r["img"] for r in recs], params, CFG.out_desc_for(IMG_ETL, aug)))
        assert np.array_equal(d.decode_named([(r["img"],) for r in recs])["image"], ref), k
    d.close()
    d = A.Decoder(dict(batch_size=1, random_seed=11, etl=[SSD_ETL, IMG_ETL], augmentation=[SSD_AUG]))
    f, states = A.ParamFactory(SSD_AUG), A.seed_slots(11, 6)
    for k in range(2):
        recs = box_window(6, seed=40 + k)
        want, _ = ssd_reference(recs, f, states, SSD_AUG)
        assert_outputs(d.decode_named(as_records(recs)), want, f"ssd window {k}")
    d.close()
