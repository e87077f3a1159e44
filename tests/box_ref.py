"""The yardstick of the box targets: aeon's boundingbox::transformer::transform_box
(src/etl_boundingbox.cpp:146-261, with boundingbox.cpp:78-163 and box.hpp:51-93) and its two loaders
(etl_boundingbox.cpp:296-318, etl_localization_ssd.cpp:116-150) restated on numpy float32 scalars.

Every arithmetic step is one operation on np.float32 operands (numpy rounds each once, to nearest
even, as the x86 SSE2 build of aeon does), in aeon's order; the box centre is summed in float64 and
narrowed, as box::xcenter does.  Integers of the params (cv::Rect, cv::Size) enter the arithmetic
through np.float32(int), the C++ int -> float conversion.  tests/test_boxes.py pins this file on aeon's
own known answers; the GPU tests then demand equality with it, bit for bit.
"""
import numpy as np

F = np.float32
EMIT_NONE, EMIT_CENTER, EMIT_MIN_OVERLAP = 0, 1, 2
ONE = F(1)


def _size(xmin, ymin, xmax, ymax):
    """box::size: inclusive, 0 for an inverted box."""
    if xmax < xmin or ymax < ymin:
        return F(0)
    w = F(F(xmax - xmin) + ONE)
    h = F(F(ymax - ymin) + ONE)
    return F(w * h)


def _coverage(b, c):
    """bbox::coverage(second): size(intersect) / size(self), 0 when the intersection is empty."""
    xmin, ymin, xmax, ymax = b
    cx0, cy0, cx1, cy1 = c
    if cx0 > xmax or cx1 < xmin or cy0 > ymax or cy1 < ymin:
        isz = F(0)  # box(): (0, 0, -1, -1)
    else:
        ix0 = cx0 if xmin < cx0 else xmin  # std::max(xmin, c.xmin)
        iy0 = cy0 if ymin < cy0 else ymin
        ix1 = cx1 if cx1 < xmax else xmax  # std::min(xmax, c.xmax)
        iy1 = cy1 if cy1 < ymax else ymax
        isz = _size(ix0, iy0, ix1, iy1)
    if isz > 0:
        with np.errstate(divide="ignore", invalid="ignore"):
            return F(isz / _size(xmin, ymin, xmax, ymax))
    return F(0)


def transform_box(box, p, emit_type=EMIT_NONE, emit_min_overlap=0.0):
    """One box (xmin, ymin, xmax, ymax) through transform_box with params p (an object with crop_x,
    crop_y, crop_w, crop_h, out_w, out_h, flip, expand_ratio, expand_x, expand_y); None = dropped."""
    xmin, ymin, xmax, ymax = (F(v) for v in box)
    if F(p.expand_ratio) > 1.0:
        ex, ey = F(int(p.expand_x)), F(int(p.expand_y))
        xmin, ymin, xmax, ymax = F(xmin + ex), F(ymin + ey), F(xmax + ex), F(ymax + ey)
    crop_x, crop_y, crop_w, crop_h = int(p.crop_x), int(p.crop_y), int(p.crop_w), int(p.crop_h)
    if emit_type != EMIT_NONE:
        cx0, cy0 = F(crop_x), F(crop_y)
        cx1, cy1 = F(crop_x + crop_w - 1), F(crop_y + crop_h - 1)
        if emit_type == EMIT_CENTER:
            xc = F(np.float64(xmin) + np.float64(F(xmax - xmin)) / 2.0)
            yc = F(np.float64(ymin) + np.float64(F(ymax - ymin)) / 2.0)
            if not (xc >= cx0 and xc <= cx1 and yc >= cy0 and yc <= cy1):
                return None
        else:
            if not (_coverage((xmin, ymin, xmax, ymax), (cx0, cy0, cx1, cy1)) >= F(emit_min_overlap)):
                return None
    cx, cy = F(crop_x), F(crop_y)
    cxe, cye = F(crop_x + crop_w), F(crop_y + crop_h)
    cw, ch = F(crop_w), F(crop_h)
    if xmax < cx or xmin >= cxe or ymax < cy or ymin >= cye:
        return None
    xmin = F(0) if xmin < cx else F(xmin - cx)
    ymin = F(0) if ymin < cy else F(ymin - cy)
    xmax = F(crop_w - 1) if xmax >= cxe else F(xmax - cx)
    ymax = F(crop_h - 1) if ymax >= cye else F(ymax - cy)
    if p.flip:
        old_xmax = xmax
        xmax = F(F(cw - xmin) - ONE)
        xmin = F(F(cw - old_xmax) - ONE)
    xs = F(F(int(p.out_w)) / cw)
    ys = F(F(int(p.out_h)) / ch)
    return (F(xmin * xs), F(ymin * ys), F(F(F(xmax + ONE) * xs) - ONE), F(F(F(ymax + ONE) * ys) - ONE))


def transform(boxes, p, emit_type=EMIT_NONE, emit_min_overlap=0.0):
    """The surviving boxes of one record, in input order: [(input index, transformed box)]."""
    out = []
    for i, b in enumerate(np.asarray(boxes, np.float32).reshape(-1, 4)):
        t = transform_box(b, p, emit_type, emit_min_overlap)
        if t is not None:
            out.append((i, t))
    return out


def load_boundingbox(boxes, p, max_boxes, item_floats=None, emit=(EMIT_NONE, 0.0)):
    """provider::boundingbox's item: the first max_boxes survivors as 4 floats each, zeros after them
    (the whole item of item_floats floats; aeon's loader defines its first max_boxes * 4)."""
    item = np.zeros(item_floats if item_floats is not None else max_boxes * 16, np.float32)
    for slot, (_, t) in enumerate(transform(boxes, p, *emit)[:max_boxes]):
        item[4 * slot:4 * slot + 4] = t
    return item


def load_ssd(boxes, labels, difficult, p, max_boxes, width, height, emit=(EMIT_NONE, 0.0)):
    """provider::localization::ssd's five outputs for one record (bbox::normalize: xmin / W, ymin / H,
    (xmax + 1) / W, (ymax + 1) / H with W, H the config's width and height)."""
    W, H = F(int(width)), F(int(height))
    kept = transform(boxes, p, *emit)[:max_boxes]
    gt = np.zeros((max_boxes, 4), np.float32)
    cls = np.zeros(max_boxes, np.int32)
    dif = np.zeros(max_boxes, np.int32)
    for slot, (i, t) in enumerate(kept):
        gt[slot] = (F(t[0] / W), F(t[1] / H), F(F(t[2] + ONE) / W), F(F(t[3] + ONE) / H))
        cls[slot] = int(labels[i])
        dif[slot] = 1 if difficult[i] else 0
    return {"image_shape": np.array([width, height], np.int32), "gt_boxes": gt,
            "gt_box_count": np.int32(len(kept)), "gt_class_count": cls, "difficult_flag": dif}


def rect(b):
    """box::rect (box.hpp:53-57): (round(xmin), round(ymin), round(width), round(height)), std::round."""
    def rnd(v):
        v = float(v)
        return int(np.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)
    xmin, ymin, xmax, ymax = (F(v) for v in b)
    return (rnd(xmin), rnd(ymin), rnd(F(F(xmax - xmin) + ONE)), rnd(F(F(ymax - ymin) + ONE)))
