"""aeon's own known answers for the box transform and loaders, restated as data from
test/test_bbox.cpp and test/test_localization_ssd.cpp (the line of each test is given).  A case is
(name, boxes xyxy, params dict, (emit type, min overlap), expected rects [box::rect() of each
survivor]); tests/test_boxes.py runs them through tests/box_ref.py, tests/test_hip_boxes.py through the
kernel."""
import numpy as np

F = np.float32

LABEL_LIST = ["person", "dog", "lion", "tiger", "eel", "puma", "rat", "tick", "flea", "bicycle", "hovercraft"]


def R(x, y, w, h):
    """create_box(cv::Rect) (test/helpers.cpp:66-75): xmax = x + w - 1."""
    return (x, y, x + w - 1, y + h - 1)


def identity(w, h):
    """make_params(width, height) of test_bbox.cpp:80-86."""
    return dict(crop_x=0, crop_y=0, crop_w=w, crop_h=h, out_w=w, out_h=h, expand_ratio=1.0)


CROP_BOXES = [R(10, 10, 10, 10), R(30, 30, 10, 10), R(50, 50, 10, 10), R(69, 31, 10, 10), R(69, 69, 10, 10),
              R(90, 35, 10, 10), R(30, 70, 10, 10), R(30, 30, 40, 40)]
GRID = [(10, 10, 10, 10), (30, 30, 10, 10), (50, 50, 10, 10), (70, 30, 10, 10), (90, 35, 10, 10), (30, 70, 10, 10),
        (70, 70, 10, 10), (30, 30, 80, 80)]
GRID_BOXES = [R(*g) for g in GRID]

EXPAND_OFF = [(10, 10), (30, 30), (50, 50), (70, 30), (90, 35), (30, 70), (70, 70), (30, 30)]
EXPAND_SIZE = [(10, 10)] * 7 + [(70, 70)]

ECFR_POS = [(0, 0), (10, 10), (30, 30), (50, 50), (70, 30), (30, 70), (70, 70)]
ECFR_SIZE = [(10, 10)] * 6 + [(20, 20)]


def _ecfr_expected():
    """boundingbox.expand_crop_flip_resize (test_bbox.cpp:555-637): its expected boxes, computed as the
    test computes them (float arithmetic on the expanded and cropped box), as rects."""
    from tests import box_ref
    xs = F(F(200) / F(150))
    ys = F(F(200) / F(150))
    out = []
    for (x, y), (w, h) in zip(ECFR_POS, ECFR_SIZE):
        e = [F(x + 100 - 50), F(y + 100 - 50), F(x + 100 - 50 + w - 1), F(y + 100 - 50 + h - 1)]
        b = (F(F(F(F(150) - e[2]) - F(1)) * xs), F(e[1] * ys),
             F(F(F(F(F(F(150) - e[0]) - F(1)) + F(1)) * xs) - F(1)), F(F(F(e[3] + F(1)) * ys) - F(1)))
        out.append(box_ref.rect(b))
    return out


def transform_cases():
    return [
        ("crop:283", CROP_BOXES, dict(identity(256, 256), crop_x=35, crop_y=35, crop_w=40, crop_h=40, out_w=40, out_h=40),
         (0, 0.0), [(0, 0, 5, 5), (15, 15, 10, 10), (34, 0, 6, 6), (34, 34, 6, 6), (0, 35, 5, 5), (0, 0, 35, 35)]),
        ("expand:335", [(x, y, x + w - 1, y + h - 1) for (x, y), (w, h) in zip(EXPAND_OFF, EXPAND_SIZE)],
         dict(crop_x=0, crop_y=0, crop_w=200, crop_h=200, out_w=200, out_h=200, expand_ratio=2.0, expand_x=50,
              expand_y=50, expand_w=200, expand_h=200),
         (0, 0.0), [(x + 50, y + 50, w, h) for (x, y), (w, h) in zip(EXPAND_OFF, EXPAND_SIZE)]),
        ("rescale:410", GRID_BOXES, dict(identity(256, 256), out_w=512, out_h=1024),
         (0, 0.0), [(x * 2, y * 4, w * 2, h * 4) for x, y, w, h in GRID]),
        ("flip:458", GRID_BOXES, dict(identity(256, 256), flip=1),
         (0, 0.0), [(256 - w - x, y, w, h) for x, y, w, h in GRID]),
        ("crop_flip:505", CROP_BOXES,
         dict(identity(256, 256), crop_x=35, crop_y=35, crop_w=40, crop_h=40, out_w=40, out_h=40, flip=1),
         (0, 0.0), [(35, 0, 5, 5), (15, 15, 10, 10), (0, 0, 6, 6), (0, 34, 6, 6), (35, 35, 5, 5), (5, 0, 35, 35)]),
        ("expand_crop_flip_resize:555", [(x, y, x + w - 1, y + h - 1) for (x, y), (w, h) in zip(ECFR_POS, ECFR_SIZE)],
         dict(crop_x=50, crop_y=50, crop_w=150, crop_h=150, out_w=200, out_h=200, flip=1, expand_ratio=3.0,
              expand_x=100, expand_y=100, expand_w=300, expand_h=300),
         (0, 0.0), _ecfr_expected()),
        ("meet_emit_constraint_center:155", [R(0, 0, 10, 10), R(10, 10, 20, 20), R(5, 5, 10, 10), R(9, 9, 2, 2)],
         dict(identity(256, 256), crop_x=6, crop_y=6, crop_w=8, crop_h=8, out_w=8, out_h=8),
         (1, 0.0), [(0, 0, 8, 8), (3, 3, 2, 2)]),
        ("meet_emit_constraint_min_overlap:190",
         [R(0, 1, 10, 1), R(0, 0, 10, 1), R(0, 2, 8, 1), R(0, 1, 12, 1), R(0, 1, 11, 1)],
         dict(identity(256, 256), crop_x=0, crop_y=1, crop_w=10, crop_h=1, out_w=10, out_h=1),
         (2, 0.9), [(0, 0, 10, 1), (0, 0, 10, 1)]),
    ]


# boundingbox.load_pad (:670) / load_full (:719): the loader over the GRID boxes as extracted (identity
# params), max_bbox_count 10 (8 boxes, then zeros) and 6 (the first six)
LOAD_CASES = [("load_pad:670", 10), ("load_full:719", 6)]

# localization_ssd.transform (test_localization_ssd.cpp:158): flip + rescale by 3, pixel boxes before
# normalisation equal bbox(...).rescale(3, 3) of the flipped boxes
SSD_TRANSFORM = dict(boxes=[(0, 0, 99, 99), (20, 40, 29, 49), (10, 20, 29, 39)],
                     params=dict(identity(100, 100), out_w=300, out_h=300, flip=1),
                     flipped=[(0, 0, 99, 99), (70, 40, 79, 49), (70, 20, 89, 39)], scale=3)

# localization_ssd.loader (:201): three transformed boxes loaded with width = height = 100
SSD_LOADER = dict(boxes=[(0.0, 0.0, 99, 99), (10, 20, 30, 40), (44.444, 55.555, 98, 99)], labels=[0, 1, 2],
                  difficult=[0, 1, 1], width=100, height=100, max_gt_boxes=64)

# boundingbox.extractor (:88) over aeon's three VOC files (tests/golden/voc)
VOC = {
    "000001.json": dict(n=2, size=(353, 500, 3),
                        boxes={0: (47, 239, 194, 370), 1: (7, 11, 351, 497)}, labels={0: 1, 1: 0},
                        difficult={0: 0, 1: 0}),
    "006637.json": dict(n=6, size=(500, 375, 3), boxes={3: (324, 109, 365, 315)}, labels={3: 0}, difficult={3: 0}),
    "009952.json": dict(n=1, size=None, boxes={}, labels={}, difficult={}),
}
