"""The yardstick of the localization_rcnn targets: aeon's localization::rcnn::transformer::transform,
sample_anchors and loader::load (src/etl_localization_rcnn.cpp:97-261, 340-428) restated on numpy float32.

Every arithmetic step is one numpy operation on float32 operands (rounded once, to nearest even, as the
x86 SSE2 build of aeon rounds), in aeon's order; box centres are summed in float64 and narrowed, as
box::xcenter does.  transform_box comes from tests/box_ref.py, the anchors from aeon_rcnn_anchors (pinned
on aeon's table by tests/test_rcnn.py), the shuffle from aeon_rcnn_sample_anchors -- the real
std::shuffle over std::minstd_rand0.  dw / dh are the float64 log of the float32 quotient, rounded to
float32: aeon's logf and the device's are each within 1 ulp of that, so a comparison allows 2 ulps
there and none anywhere else.  tests/test_rcnn.py pins this file on aeon's own known answer; the GPU
tests then demand equality with it.
"""
import numpy as np

import aeon_amd as A
from tests import box_ref as B

F = np.float32
ONE = F(1)


def image_scale(p, info, fixed_scaling_factor):
    """(im_scale, im_w, im_h) of transformer::transform for params p."""
    if fixed_scaling_factor > 0:
        s = F(fixed_scaling_factor)
    else:
        s = F(A.calculate_scale(int(p.crop_w), int(p.crop_h), info["width"], info["height"]))
    return s, A.unbiased_round(float(F(F(int(p.crop_w)) * s))), A.unbiased_round(float(F(F(int(p.crop_h)) * s)))


def inside(anchors, im_w, im_h):
    """anchor::inside_image_bounds as a mask over all anchors."""
    a = anchors
    return (a[:, 0] >= 0) & (a[:, 1] >= 0) & (a[:, 2] < F(im_w)) & (a[:, 3] < F(im_h))


def bbox_overlaps(a, g):
    """(N, K) float32 overlaps of anchors a (N, 4) with gt boxes g (K, 4)."""
    ax0, ay0, ax1, ay1 = (a[:, i][:, None] for i in range(4))
    gx0, gy0, gx1, gy1 = (g[:, i][None, :] for i in range(4))
    garea = ((g[:, 2] - g[:, 0] + ONE) * (g[:, 3] - g[:, 1] + ONE))[None, :]
    iw = np.minimum(ax1, gx1) - np.maximum(ax0, gx0) + ONE
    ih = np.minimum(ay1, gy1) - np.maximum(ay0, gy0) + ONE
    aarea = (ax1 - ax0 + ONE) * (ay1 - ay0 + ONE)
    with np.errstate(divide="ignore", invalid="ignore"):
        ua = aarea + garea - iw * ih
        ov = iw * ih / ua
    out = np.where((iw > 0) & (ih > 0), ov, F(0)).astype(np.float32)
    assert out.dtype == np.float32 and iw.dtype == np.float32 and ua.dtype == np.float32
    return out


def _center(lo, hi):
    return (lo.astype(np.float64) + (hi - lo).astype(np.float64) / 2.0).astype(np.float32)


def compute_targets(gt, rp):
    """transformer::compute_targets for paired boxes gt, rp (n, 4): (dx, dy, dw, dh, qw, qh) with qw, qh the
    float32 quotients the logarithms are taken of."""
    gt, rp = np.asarray(gt, np.float32).reshape(-1, 4), np.asarray(rp, np.float32).reshape(-1, 4)
    rw, rh = rp[:, 2] - rp[:, 0] + ONE, rp[:, 3] - rp[:, 1] + ONE
    dx = (_center(gt[:, 0], gt[:, 2]) - _center(rp[:, 0], rp[:, 2])) / rw
    dy = (_center(gt[:, 1], gt[:, 3]) - _center(rp[:, 1], rp[:, 3])) / rh
    qw, qh = (gt[:, 2] - gt[:, 0] + ONE) / rw, (gt[:, 3] - gt[:, 1] + ONE) / rh
    dw, dh = np.log(qw.astype(np.float64)).astype(np.float32), np.log(qh.astype(np.float64)).astype(np.float32)
    return dx, dy, dw, dh, qw, qh


def transform(info, anchors, boxes, p, emit=(B.EMIT_NONE, 0.0), fixed_scaling_factor=-1.0):
    """transformer::transform up to the labels: dict(labels (A,) int32 on the whole canvas, gt (K, 4),
    kept = input indices of the K survivors, argmax (A,) gt index per anchor (-1 outside), row_max, overlaps
    of the inside anchors, idx_inside, im_scale, im_w, im_h)."""
    s, im_w, im_h = image_scale(p, info, fixed_scaling_factor)
    kept = B.transform(boxes, p, *emit)
    gt = np.array([t for _, t in kept], np.float32).reshape(-1, 4)
    A_ = len(anchors)
    labels = np.full(A_, -1, np.int32)
    argmax = np.full(A_, -1, np.int64)
    ins = np.flatnonzero(inside(anchors, im_w, im_h))
    ov = bbox_overlaps(anchors[ins], gt)
    row_max = np.zeros(len(ins), np.float32)
    if len(gt):  # with no gt box aeon's map-back loop copies nothing: every label stays -1
        row_max = np.maximum(F(0), ov.max(axis=1))
        col_max = np.maximum(F(0), ov.max(axis=0)) if len(ins) else np.zeros(len(gt), np.float32)
        lab = np.full(len(ins), -1, np.int32)
        lab[row_max < F(info["negative_overlap"])] = 0
        lab[(ov == col_max[None, :]).any(axis=1)] = 1
        lab[row_max >= F(info["positive_overlap"])] = 1
        labels[ins] = lab
        # the first gt box attaining the row maximum; index 0 when every overlap is 0
        argmax[ins] = np.where(row_max > 0, (ov == row_max[:, None]).argmax(axis=1), 0)
    return dict(labels=labels, gt=gt, kept=[i for i, _ in kept], argmax=argmax, idx_inside=ins, overlaps=ov,
                row_max=row_max, im_scale=s, im_w=im_w, im_h=im_h)


def load(info, anchors, t, sampled, labels_in, difficult_in):
    """loader::load: the ten outputs of one record as aeon shapes them, plus "quotients" (the float32
    arguments of dw / dh's logarithms, for the ulp test)."""
    A_, m = len(anchors), info["max_gt_boxes"]
    bbt, bbm = np.zeros(4 * A_, np.float32), np.zeros(4 * A_, np.float32)
    lf = np.concatenate([np.ones(A_, np.int32), np.zeros(A_, np.int32)])
    lm = np.zeros(2 * A_, np.int32)
    quot = np.zeros(4 * A_, np.float32)
    idx = np.asarray(sampled, np.int64)
    if len(idx):
        dx, dy, dw, dh, qw, qh = compute_targets(t["gt"][t["argmax"][idx]], anchors[idx])
        for plane, v in enumerate((dx, dy, dw, dh)):
            bbt[idx + plane * A_] = v
        quot[idx + 2 * A_], quot[idx + 3 * A_] = qw, qh
        fg = idx[t["labels"][idx] == 1]
        lf[fg], lf[fg + A_] = 0, 1
        for plane in range(4):
            bbm[fg + plane * A_] = ONE
        lm[idx], lm[idx + A_] = 1, 1
    k = min(m, len(t["gt"]))
    gtb, cls, dif = np.zeros((m, 4), np.float32), np.zeros((m, 1), np.int32), np.zeros((m, 1), np.int32)
    gtb[:k] = t["gt"][:k]
    for slot, i in enumerate(t["kept"][:k]):
        cls[slot, 0] = int(labels_in[i])
        dif[slot, 0] = 1 if difficult_in[i] else 0
    return {"bbtargets": bbt, "bbtargets_mask": bbm, "labels_flat": lf.reshape(1, -1), "labels_mask": lm.reshape(-1, 1),
            "image_shape": np.array([[t["im_w"]], [t["im_h"]]], np.int32), "gt_boxes": gtb,
            "gt_box_count": np.array([[k]], np.int32), "gt_class_count": cls,
            "image_scale": np.array([[t["im_scale"]]], np.float32), "difficult_flag": dif, "quotients": quot}


def record(config, anchors, rec, p, state=None, shuffle=True, emit=(B.EMIT_NONE, 0.0), fixed_scaling_factor=-1.0,
           info=None):
    """One record through transform, sample_anchors and load.  rec = (boxes, labels, difficult); state: a
    one-element np.uint32 array (the engine's state word), advanced in place.  Returns (outputs, transform
    dict, sampled anchor indices)."""
    info = info or A.rcnn_config_info(config)
    boxes, labels, difficult = rec
    t = transform(info, anchors, boxes, p, emit, fixed_scaling_factor)
    sampled = A.rcnn_sample_anchors(t["labels"], info["rois_per_image"], info["num_fg"], shuffle, state)
    return load(info, anchors, t, sampled, labels, difficult), t, sampled


def ulp_distance(a, b):
    """Distance in float32 ulps between equally shaped arrays (monotone integer order of the patterns)."""
    def order(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(order(a) - order(b))


def assert_equal(got, want, what=""):
    """The ten outputs bit for bit, but dw / dh (planes 2 and 3 of bbtargets) within 2 ulps."""
    A_ = want["bbtargets"].size // 4
    for name in A.RCNN_OUTPUTS:
        g = np.ascontiguousarray(got[name]).reshape(-1)
        w = np.ascontiguousarray(want[name]).reshape(-1)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        if name == "bbtargets":
            assert np.array_equal(g[:2 * A_].view(np.uint32), w[:2 * A_].view(np.uint32)), (what, name, "dx / dy")
            d = ulp_distance(g[2 * A_:], w[2 * A_:])
            assert d.max() <= 2, (what, name, "dw / dh", int(d.max()))
        else:
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (what, name)
