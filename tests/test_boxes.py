"""CPU: the host half of the boundingbox / localization_ssd targets -- the metadata extractor
(aeon_box_extract), the factory's emit constraint, the two ETL configs and the decoder's output names,
order, shapes and types for them -- and the yardstick the GPU tests compare the kernel with
(tests/box_ref.py), pinned on aeon's own known answers (tests/box_cases.py, restated from
test/test_bbox.cpp and test/test_localization_ssd.cpp).  The draws of a [localization_ssd, image]
window need the records' metadata and so a decode window: their routing is checked in
tests/test_hip_boxes.py."""
import json
import os

import numpy as np
import pytest

import aeon_amd as A
from tests import box_cases as C
from tests import box_ref as B

F = np.float32
VOC_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voc")


def voc(name):
    return open(os.path.join(VOC_DIR, name), "rb").read()


def metadata(boxes, names, width=256, height=256, **extra):
    """create_metadata / create_box of aeon's tests (test/helpers.cpp:66-92)."""
    objs = [dict({"bndbox": {"xmax": b[2], "xmin": b[0], "ymax": b[3], "ymin": b[1]}, "name": n}, **extra)
            for b, n in zip(boxes, names)]
    return json.dumps({"object": objs, "size": {"depth": 3, "height": height, "width": width}})


# ---- box_ref against aeon's known answers -------------------------------------------------------
@pytest.mark.parametrize("case", C.transform_cases(), ids=lambda c: c[0])
def test_ref_transform_known_answers(case):
    _, boxes, params, emit, expect = case
    kept = B.transform(boxes, A.aug_params(**params), *emit)
    assert [B.rect(t) for _, t in kept] == expect


@pytest.mark.parametrize("name,max_boxes", C.LOAD_CASES)
def test_ref_boundingbox_loader_known_answers(name, max_boxes):
    item = B.load_boundingbox(C.GRID_BOXES, A.aug_params(**C.identity(256, 256)), max_boxes)
    n = min(max_boxes, len(C.GRID_BOXES))
    assert item[:4 * n].astype(int).tolist() == [v for b in C.GRID_BOXES[:n] for v in b]
    assert not item[4 * n:].any() and item.size == max_boxes * 16


def test_ref_ssd_transform_known_answer():
    t = C.SSD_TRANSFORM
    kept = B.transform(t["boxes"], A.aug_params(**t["params"]))
    s = F(t["scale"])
    want = [(F(b[0] * s), F(b[1] * s), F(F(F(b[2] + 1) * s) - 1), F(F(F(b[3] + 1) * s) - 1))
            for b in np.asarray(t["flipped"], np.float32)]
    assert [k for _, k in kept] == want


def test_ref_ssd_loader_known_answer():
    t = C.SSD_LOADER
    out = B.load_ssd(t["boxes"], t["labels"], t["difficult"], A.aug_params(**C.identity(t["width"], t["height"])),
                     t["max_gt_boxes"], t["width"], t["height"])
    assert out["image_shape"].tolist() == [100, 100] and out["gt_box_count"] == 3
    for i, b in enumerate(np.asarray(t["boxes"], np.float32)):
        want = [F(b[0] / F(100)), F(b[1] / F(100)), F(F(b[2] + F(1)) / F(100)), F(F(b[3] + F(1)) / F(100))]
        assert out["gt_boxes"][i].tolist() == want
    assert out["gt_class_count"][:3].tolist() == [0, 1, 2] and out["difficult_flag"][:3].tolist() == [0, 1, 1]
    assert not out["gt_boxes"][3:].any() and not out["gt_class_count"][3:].any() and not out["difficult_flag"][3:].any()


# ---- extractor -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.VOC))
def test_extractor_voc_fixtures(name):
    """boundingbox.extractor (test_bbox.cpp:88-153)."""
    want = C.VOC[name]
    m = A.box_extract(C.LABEL_LIST, voc(name))
    assert len(m["boxes"]) == len(m["labels"]) == len(m["difficult"]) == want["n"]
    if want["size"]:
        assert (m["width"], m["height"], m["depth"]) == want["size"]
    for i, b in want["boxes"].items():
        assert tuple(m["boxes"][i]) == b and m["labels"][i] == want["labels"][i]
        assert m["difficult"][i] == want["difficult"][i]
    assert m["boxes"].dtype == np.float32 and m["labels"].dtype == np.int32


def test_extractor_metadata_and_labels():
    """boundingbox.bbox (test_bbox.cpp:255-281): labels through class_names, fractional coordinates as
    floats, difficult / truncated optional."""
    boxes = [C.R(0, 0, 10, 15), C.R(10, 10, 12, 13), (100.25, 100.5, 219.75, 229.0)]
    m = A.box_extract(C.LABEL_LIST, metadata(boxes, ["rat", "flea", "tick"]))
    assert m["labels"].tolist() == [6, 8, 7] and m["difficult"].tolist() == [0, 0, 0]
    assert m["boxes"].tolist() == [[0, 0, 9, 14], [10, 10, 21, 22], [100.25, 100.5, 219.75, 229.0]]
    assert (m["width"], m["height"], m["depth"]) == (256, 256, 3)
    m = A.box_extract(C.LABEL_LIST, metadata(boxes[:2], ["rat", "flea"], difficult=True, truncated=False))
    assert m["difficult"].tolist() == [1, 1]


def test_extractor_zero_boxes_and_many_boxes():
    m = A.box_extract(C.LABEL_LIST, metadata([], []))
    assert m["boxes"].shape == (0, 4) and m["labels"].size == 0
    boxes = [(i, i + 1, i + 2, i + 3) for i in range(300)]  # above the binding's first capacity
    m = A.box_extract(C.LABEL_LIST, metadata(boxes, ["eel"] * 300))
    assert m["boxes"].tolist() == [list(map(float, b)) for b in boxes] and m["labels"].tolist() == [4] * 300


def _drop(text, path):
    j = json.loads(text)
    d = j
    for k in path[:-1]:
        d = d[k]
    del d[path[-1]]
    return json.dumps(j)


@pytest.mark.parametrize("path,message", [
    (("object",), "'object' missing from metadata"),
    (("size",), "'size' missing from metadata"),
    (("size", "width"), "'width' missing from metadata"),
    (("size", "height"), "'height' missing from metadata"),
    (("size", "depth"), "'depth' missing from metadata"),
    (("object", 0, "bndbox", "xmax"), "'xmax' missing from metadata"),
    (("object", 0, "bndbox", "xmin"), "'xmin' missing from metadata"),
    (("object", 0, "bndbox", "ymax"), "'ymax' missing from metadata"),
    (("object", 0, "bndbox", "ymin"), "'ymin' missing from metadata"),
    (("object", 0, "name"), "'name' missing from metadata"),
])
def test_extractor_error_texts(path, message):
    text = _drop(metadata([C.R(1, 2, 3, 4)], ["dog"]), path)
    with pytest.raises(A.AeonHipError) as e:
        A.box_extract(C.LABEL_LIST, text)
    assert e.value.code == A.AEON_HIP_EINVAL and str(e.value).endswith(message)


def test_extractor_errors():
    """boundingbox.extractor_error / extractor_missing_label (test_bbox.cpp:237-253)."""
    with pytest.raises(A.AeonHipError) as e:
        A.box_extract(C.LABEL_LIST, "{}")
    assert e.value.code == A.AEON_HIP_EINVAL
    with pytest.raises(A.AeonHipError) as e:
        A.box_extract(["monkey", "tuna"], voc("009952.json"))
    name = json.loads(voc("009952.json"))["object"][0]["name"]
    assert str(e.value).endswith(f"label '{name}' not found in metadata label list")
    for bad in ("", "[", '{"object": [], "size": {"width": "x", "height": 1, "depth": 3}}',
                metadata([("a", 1, 2, 3)], ["dog"]), metadata([C.R(1, 2, 3, 4)], ["dog"], difficult=1)):
        with pytest.raises(A.AeonHipError) as e:
            A.box_extract(C.LABEL_LIST, bad)
        assert e.value.code == A.AEON_HIP_EINVAL, bad


def test_extract_cap_reports_full_count():
    """aeon_box_extract writes at most cap boxes and reports all of them."""
    import ctypes
    text = metadata([(i, i, i + 5, i + 5) for i in range(9)], ["dog"] * 9).encode()
    boxes, labels, diff = np.full((4, 4), -1, np.float32), np.full(4, -1, np.int32), np.full(4, -1, np.int32)
    n = ctypes.c_int()
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    rc = A.lib().aeon_box_extract(json.dumps(C.LABEL_LIST).encode(), text, len(text), None, None, None,
                                  boxes.ctypes.data_as(fp), labels.ctypes.data_as(ip), diff.ctypes.data_as(ip), 3,
                                  ctypes.byref(n))
    assert rc == 0 and n.value == 9
    assert boxes[:3].tolist() == [[i, i, i + 5, i + 5] for i in range(3)] and (boxes[3] == -1).all()
    assert labels.tolist() == [1, 1, 1, -1] and diff.tolist() == [0, 0, 0, -1]


# ---- emit constraint -----------------------------------------------------------------------------
def test_param_factory_emit():
    assert A.ParamFactory({"type": "image"}).emit() == (A.EMIT_NONE, 0.0)
    assert A.ParamFactory({"type": "image", "emit_constraint_type": "center"}).emit() == (A.EMIT_CENTER, 0.0)
    t, m = A.ParamFactory({"type": "image", "emit_constraint_type": "MIN_OVERLAP",
                           "emit_constraint_min_overlap": 0.9}).emit()
    assert t == A.EMIT_MIN_OVERLAP and m == float(F(0.9))
    assert A.ParamFactory({"type": "image", "emit_constraint_type": ""}).emit()[0] == A.EMIT_NONE
    with pytest.raises(A.AeonHipError) as e:
        A.ParamFactory({"type": "image", "emit_constraint_type": "centre"})
    assert e.value.code == A.AEON_HIP_EINVAL and "Invalid emit constraint type" in str(e.value)


# ---- ETL configs and the decoder's outputs (no device: the context is made by the first window) -----
CLASSES = ["bicycle", "person"]
SSD_ETL = {"type": "localization_ssd", "height": 375, "width": 500, "max_gt_boxes": 64, "class_names": CLASSES}
BBOX_ETL = {"type": "boundingbox", "height": 100, "width": 150, "max_bbox_count": 10, "class_names": CLASSES}
IMAGE_ETL = {"type": "image", "height": 375, "width": 500, "channel_major": False}
AUG = {"type": "image", "flip_enable": True}


def _outputs(etl, **extra):
    d = A.Decoder(dict(batch_size=2, etl=etl, augmentation=[AUG], **extra))
    return [(o["name"], o["shape"], o["dtype"], o["item_bytes"]) for o in d.outputs], d


def test_outputs_ssd_then_image():
    """localization_ssd.provider (test_localization_ssd.cpp:49-67): six buffers, the five of the ssd
    provider first, in aeon's order."""
    outs, d = _outputs([SSD_ETL, IMAGE_ETL])
    assert d.n_inputs == 2
    assert outs == [("image_shape", (2, 1), np.int32, 8), ("gt_boxes", (64, 4), np.float32, 1024),
                    ("gt_box_count", (1, 1), np.int32, 4), ("gt_class_count", (64, 1), np.int32, 256),
                    ("difficult_flag", (64, 1), np.int32, 256), ("image", (375, 500, 3), np.uint8, 375 * 500 * 3)]


def test_outputs_image_then_boundingbox():
    """boundingbox::config's shape {max_bbox_count, 4 * sizeof(float)} of output_type
    (etl_boundingbox.cpp:41), named through create_name."""
    outs, _ = _outputs([IMAGE_ETL, dict(BBOX_ETL, name="gt")])
    assert outs == [("image", (375, 500, 3), np.uint8, 375 * 500 * 3), ("gt.boundingbox", (10, 16), np.float32, 640)]
    outs, _ = _outputs([IMAGE_ETL, dict(BBOX_ETL, output_type="uint8_t")])
    assert outs[1] == ("boundingbox", (10, 16), np.uint8, 160)
    outs, _ = _outputs([IMAGE_ETL, dict(SSD_ETL, name="t", max_gt_boxes=3)])
    assert [o[0] for o in outs[1:]] == ["t.image_shape", "t.gt_boxes", "t.gt_box_count", "t.gt_class_count",
                                        "t.difficult_flag"]
    assert outs[2][1] == (3, 4)
    outs, _ = _outputs([IMAGE_ETL, {k: v for k, v in SSD_ETL.items() if k != "max_gt_boxes"}])
    assert outs[2][1] == (64, 4)  # max_gt_boxes defaults to 64


@pytest.mark.parametrize("etl,message", [
    ({k: v for k, v in BBOX_ETL.items() if k != "max_bbox_count"}, "'max_bbox_count' not set"),
    ({k: v for k, v in BBOX_ETL.items() if k != "class_names"}, "'class_names' not set"),
    ({k: v for k, v in BBOX_ETL.items() if k != "height"}, "'height' not set"),
    ({k: v for k, v in SSD_ETL.items() if k != "width"}, "'width' not set"),
    ({k: v for k, v in SSD_ETL.items() if k != "class_names"}, "'class_names' not set"),
    (dict(SSD_ETL, width=0), "invalid width"),
    (dict(SSD_ETL, height=-1), "invalid height"),
    (dict(SSD_ETL, max_gt_boxes=0), "invalid max_gt_boxes"),
    (dict(SSD_ETL, class_names=[]), "class_names cannot be empty"),
    (dict(SSD_ETL, max_gt_boxs=3), "config element {max_gt_boxs} is not understood in localization_ssd, "
                                   "did you mean {max_gt_boxes}?"),
    (dict(BBOX_ETL, max_bbox_cnt=3), "config element {max_bbox_cnt} is not understood in bbox"),
    (dict(BBOX_ETL, output_type="float16"), "'output_type' out of range"),
    (dict(SSD_ETL, output_type="float"), "is not understood in localization_ssd"),
])
def test_box_config_validation(etl, message):
    with pytest.raises(A.AeonHipError) as e:
        A.Decoder(dict(batch_size=2, etl=[etl, IMAGE_ETL], augmentation=[AUG]))
    assert e.value.code == A.AEON_HIP_EINVAL and message in str(e.value)


def test_emit_constraint_is_a_config_error():
    with pytest.raises(A.AeonHipError) as e:
        A.Decoder(dict(batch_size=2, etl=[SSD_ETL, IMAGE_ETL],
                       augmentation=[dict(AUG, emit_constraint_type="centre")]))
    assert e.value.code == A.AEON_HIP_EINVAL and "Invalid emit constraint type" in str(e.value)


def test_record_elem_entries_refuse_box_configs():
    """aeon_decoder_decode / aeon_decoder_draw_params take aeon_record_elem, which has no byte size for
    the metadata: AEON_HIP_EINVAL before anything runs."""
    _, d = _outputs([SSD_ETL, IMAGE_ETL])
    img = np.zeros((375, 500, 3), np.uint8)
    with pytest.raises(A.AeonHipError) as e:
        d.decode([(img, img)])  # no bytes element: the aeon_record_elem entry
    assert e.value.code == A.AEON_HIP_EINVAL and "aeon_decoder_decode_encoded" in str(e.value)
    with pytest.raises(A.AeonHipError) as e:
        d.draw_params([(500, 375)])
    assert e.value.code == A.AEON_HIP_EINVAL
