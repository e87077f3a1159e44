"""CPU: the host half of the localization_rcnn targets and their yardstick.

* aeon_rcnn_anchors equals aeon's table (test/test_localization_rcnn.cpp generate_anchors, as numbers in
  tests/golden/rcnn_kat.json) and base anchor + shift for every anchor, in aeon's order.
* The config: defaults, rejections, and the ten buffer names and shapes a decoder reports.
* tests/rcnn_ref.py reproduces aeon's loader known answer (006637.json at 1000 x 1000, fixed_scaling_factor
  1.6, no crop, no flip, no shuffle): the index lists exactly, the targets within aeon's own 1e-5, and the
  loader_zero_gt_boxes behaviour; compute_targets' pairs.
* `make -C aeon_amd/csrc sanitize_rcnn` builds tests/sanitize/rcnn_driver.cpp (a stand-alone program over
  rcnn_host.cpp and the shuffle header the device shares, compiled for the host) under AddressSanitizer +
  UndefinedBehaviorSanitizer; it must end clean, with the header equal to std::shuffle for every n from 0 to
  300 and for 46340, 46341 and 60000, in permutation and engine end state, from three seeds."""
import json
import os
import subprocess

import numpy as np
import pytest

import aeon_amd as A
from tests import box_cases as C
from tests import rcnn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "aeon_amd", "csrc", "build_sanitize", "rcnn_driver")
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "rcnn_kat.json")))
VOC = os.path.join(ROOT, "tests", "golden", "voc", "006637.json")
AEON_CFG = {"type": "localization_rcnn", "height": 1000, "width": 1000, "class_names": C.LABEL_LIST, "max_gt_boxes": 64}
AEON_AUG = {"type": "image", "flip_enable": False, "crop_enable": False, "fixed_aspect_ratio": True,
            "fixed_scaling_factor": 1.6}
F = np.float32


def test_anchors_equal_aeons_table():
    a = A.rcnn_anchors(AEON_CFG)
    assert a.shape == (KAT["total_anchors"], 4) == (9 * 62 * 62, 4)
    base = np.array(KAT["base_anchors"], np.float32)
    assert np.array_equal(a[::62 * 62], base)
    shift = (np.arange(62, dtype=np.float64) / np.float64(F(1.0 / 16.0))).astype(np.float32)
    sy, sx = np.meshgrid(shift, shift, indexing="ij")  # shift rows, then shift columns
    s = np.stack([sx, sy, sx, sy], -1).reshape(-1, 4)
    assert np.array_equal(a, (s[None] + base[:, None]).reshape(-1, 4))


def test_anchors_of_small_grids():
    cfg = dict(AEON_CFG, height=48, width=80, scales=[1, 2, 3])
    a = A.rcnn_anchors(cfg)
    assert a.shape == (135, 4) and A.rcnn_config_info(cfg)["total_anchors"] == 135
    # ratio 1, scale 1: the 16 x 16 window itself, at the origin and one column to the right
    assert a[3 * 15].tolist() == [0, 0, 15, 15] and a[3 * 15 + 1].tolist() == [16, 0, 31, 15]
    assert a[3 * 15 + 5].tolist() == [0, 16, 15, 31]  # 5 columns per row


def test_config_defaults_and_rejections():
    info = A.rcnn_config_info({"height": 1000, "width": 1000, "class_names": ["a"]})
    assert (info["rois_per_image"], info["num_fg"], info["max_gt_boxes"], info["total_anchors"]) == (256, 128, 64, 34596)
    assert info["negative_overlap"] == F(0.3) and info["positive_overlap"] == F(0.7)
    assert (info["max_total_anchors"], info["max_rois_per_image"]) == (65536, 1024)
    assert A.rcnn_config_info(dict(AEON_CFG, rois_per_image=16, foreground_fraction=0.25))["num_fg"] == 4
    for missing in ("height", "width", "class_names"):
        cfg = {k: v for k, v in AEON_CFG.items() if k != missing}
        with pytest.raises(A.AeonHipError) as e:
            A.rcnn_config_info(cfg)
        assert e.value.code == A.AEON_HIP_EINVAL and missing in str(e.value)
    for key in ("negative_overlap", "positive_overlap", "foreground_fraction"):
        for bad in (-0.1, 1.5):
            with pytest.raises(A.AeonHipError) as e:
                A.rcnn_config_info(dict(AEON_CFG, **{key: bad}))
            assert e.value.code == A.AEON_HIP_EINVAL and key in str(e.value)
        A.rcnn_config_info(dict(AEON_CFG, **{key: 1.0}))
    with pytest.raises(A.AeonHipError) as e:
        A.rcnn_config_info(dict(AEON_CFG, max_gt_box=3))
    assert "max_gt_box" in str(e.value) and "not understood" in str(e.value)


def test_decoder_reports_the_ten_buffers():
    img = {"type": "image", "height": 1000, "width": 1000}
    d = A.Decoder(dict(batch_size=2, etl=[dict(AEON_CFG, name="rpn"), img]))
    A_ = 34596
    want = [("bbtargets", (4 * A_,), np.float32), ("bbtargets_mask", (4 * A_,), np.float32),
            ("labels_flat", (1, 2 * A_), np.int32), ("labels_mask", (2 * A_, 1), np.int32),
            ("image_shape", (2, 1), np.int32), ("gt_boxes", (64, 4), np.float32), ("gt_box_count", (1, 1), np.int32),
            ("gt_class_count", (64, 1), np.int32), ("image_scale", (1, 1), np.float32),
            ("difficult_flag", (64, 1), np.int32)]
    got = [(o["name"], o["shape"], o["dtype"]) for o in d.outputs[:10]]
    assert got == [("rpn." + n, s, t) for n, s, t in want]
    assert tuple(n for n, _, _ in want) == A.RCNN_OUTPUTS
    assert d.outputs[10]["name"] == "image" and len(d.outputs) == 11
    d.close()
    d = A.Decoder(dict(batch_size=2, etl=[AEON_CFG, img]))
    assert [o["name"] for o in d.outputs[:10]] == list(A.RCNN_OUTPUTS)
    d.close()
    # the other ETL types of aeon stay outside this stage
    for other in ("label", "blob", "video", "char_map", "label_map"):
        with pytest.raises(A.AeonHipError) as e:
            A.Decoder(dict(batch_size=2, etl=[{"type": other}]))
        assert "outside the HIP image stage" in str(e.value)
    with pytest.raises(A.AeonHipError) as e:
        A.Decoder(dict(batch_size=2, etl=[dict(AEON_CFG, bogus=1), img]))
    assert e.value.code == A.AEON_HIP_EINVAL
    with pytest.raises(A.AeonHipError) as e:  # 9 * 94 * 94 anchors: above the stated limit
        A.Decoder(dict(batch_size=2, etl=[dict(AEON_CFG, height=1504, width=1504), img]))
    assert e.value.code == A.AEON_HIP_EUNSUPPORTED and "total_anchors" in str(e.value)


@pytest.fixture(scope="module")
def aeon_record():
    meta = A.box_extract(C.LABEL_LIST, open(VOC, "rb").read())
    p = A.ParamFactory(AEON_AUG).make_params(np.array([1], np.uint32), meta["width"], meta["height"], 1000, 1000)
    return meta, p, A.rcnn_anchors(AEON_CFG)


def test_reference_reproduces_aeons_loader_known_answer(aeon_record):
    meta, p, anchors = aeon_record
    L = KAT["loader"]
    assert (p.crop_x, p.crop_y, p.crop_w, p.crop_h, p.flip) == (0, 0, 500, 375, 0)
    out, t, sampled = R.record(AEON_CFG, anchors, (meta["boxes"], meta["labels"], meta["difficult"]), p, shuffle=False,
                               fixed_scaling_factor=1.6)
    assert sampled.tolist() == L["fg_idx"] + L["bg_idx"]
    A_ = len(anchors)
    assert np.flatnonzero(out["labels_mask"]).tolist() == sorted(L["labels_mask_idx"])
    fg = np.array(L["fg_idx"])
    want_flat = np.concatenate([np.ones(A_, np.int32), np.zeros(A_, np.int32)])
    want_flat[fg], want_flat[fg + A_] = 0, 1
    assert np.array_equal(out["labels_flat"].reshape(-1), want_flat)
    assert np.flatnonzero(out["bbtargets_mask"]).tolist() == L["bbox_mask_index"]
    assert set(out["bbtargets_mask"][L["bbox_mask_index"]].tolist()) == {1.0}
    want_t = np.zeros(4 * A_, np.float64)
    for i, v in L["bbox_targets"]:
        want_t[i] = v
    assert len(L["bbox_targets"]) == 4 * 256
    assert np.abs(out["bbtargets"].astype(np.float64) - want_t).max() <= L["tolerance"]
    assert out["image_shape"].reshape(-1).tolist() == L["image_shape"] and out["gt_box_count"].item() == L["gt_box_count"]
    assert out["image_scale"].item() == F(1.6)
    s = F(1.6)
    for i, b in enumerate(meta["boxes"]):  # aeon's own expectation of gt_boxes
        assert out["gt_boxes"][i].tolist() == [F(b[0] * s), F(b[1] * s), F(F(F(b[2] + 1) * s) - 1), F(F(F(b[3] + 1) * s) - 1)]
        assert out["gt_class_count"][i, 0] == meta["labels"][i] and out["difficult_flag"][i, 0] == meta["difficult"][i]
    assert not out["gt_boxes"][6:].any() and not out["gt_class_count"][6:].any()


def test_reference_zero_gt_boxes(aeon_record):
    """localization_rcnn.loader_zero_gt_boxes: a crop to the image's corner keeps no box; nothing is
    labelled (aeon's map-back loop stops at once), nothing sampled, every buffer at its fill value."""
    meta, _, anchors = aeon_record
    aug = {"type": "image", "flip_enable": False, "scale": [0.1, 0.1]}
    p = A.ParamFactory(aug).make_params(np.array([1], np.uint32), meta["width"], meta["height"], 1000, 1000)
    p.crop_x = p.crop_y = 0
    state = np.array([77], np.uint32)
    out, t, sampled = R.record(AEON_CFG, anchors, (meta["boxes"], meta["labels"], meta["difficult"]), p, state=state)
    assert len(t["gt"]) == 0 and len(sampled) == 0 and state[0] == 77
    assert (t["labels"] == -1).all() and len(t["idx_inside"]) > 0
    A_ = len(anchors)
    assert not out["bbtargets"].any() and not out["bbtargets_mask"].any() and not out["labels_mask"].any()
    assert out["labels_flat"].reshape(-1).tolist() == [1] * A_ + [0] * A_
    assert out["gt_box_count"].item() == 0 and not out["gt_boxes"].any()


def test_reference_compute_targets():
    for case in KAT["compute_targets"]:
        dx, dy, dw, dh, _, _ = R.compute_targets([case["gt"]], [case["rp"]])
        got = np.array([dx[0], dy[0], dw[0], dh[0]], np.float64)
        assert np.abs(got - np.array(case["expected"])).max() <= KAT["compute_targets_tolerance"]


def test_host_sampling_without_shuffle_and_cuts():
    labels = np.array([1, 0, -1, 2, 0, 0, 1, 0, 1], np.int32)
    assert A.rcnn_sample_anchors(labels, 6, 2, shuffle=False).tolist() == [0, 3, 1, 4, 5, 7]
    assert A.rcnn_sample_anchors(labels, 16, 8, shuffle=False).tolist() == [0, 3, 6, 8, 1, 4, 5, 7]
    assert A.rcnn_sample_anchors(labels, 3, 3, shuffle=False).tolist() == [0, 3, 6]
    st = np.array([9], np.uint32)
    a = A.rcnn_sample_anchors(labels, 6, 2, True, st)
    assert st[0] != 9 and set(a[:2]) <= {0, 3, 6, 8} and set(a[2:]) <= {1, 4, 5, 7} and len(set(a)) == 6
    st2 = np.array([9], np.uint32)
    assert A.rcnn_sample_anchors(labels, 6, 2, True, st2).tolist() == a.tolist() and st2[0] == st[0]


def test_engine_words_congruent_to_zero_are_taken_as_one():
    """minstd_rand0::seed maps 0, 2^31 - 1 and 2^32 - 2 to 1: the host sampling gives what state 1 gives."""
    labels = np.array([1, 0, 0, 1, 0, 0, 1, 0, 0, 0, 1], np.int32)
    one = np.array([1], np.uint32)
    want = A.rcnn_sample_anchors(labels, 8, 3, True, one).tolist()
    for word in (0, 0x7FFFFFFF, 0xFFFFFFFE):
        st = np.array([word], np.uint32)
        assert A.rcnn_sample_anchors(labels, 8, 3, True, st).tolist() == want and st[0] == one[0]
        st = np.array([word], np.uint32)  # no draw: the word comes back as the engine holds it
        A.rcnn_sample_anchors(labels[:1], 8, 3, True, st)
        assert st[0] == 1


def test_config_refusals_of_this_build_are_unsupported():
    """What aeon would take and only this build cannot is AEON_HIP_EUNSUPPORTED; a scaling_factor above 1, a
    large base_size and many ratios are taken."""
    for bad in (dict(width=(1 << 24) + 1), dict(height=(1 << 24) + 1), dict(max_gt_boxes=(1 << 24) + 1),
                dict(scaling_factor=1e6)):
        with pytest.raises(A.AeonHipError) as e:
            A.rcnn_config_info(dict(AEON_CFG, **bad))
        assert e.value.code == A.AEON_HIP_EUNSUPPORTED, bad
    assert A.rcnn_config_info(dict(AEON_CFG, height=16, width=16, scaling_factor=2.0))["total_anchors"] == 9 * 32 * 32
    assert A.rcnn_anchors(dict(AEON_CFG, height=16, width=16, scaling_factor=2.0))[1].tolist() == [-83.5, -40, 99.5, 55]
    assert A.rcnn_config_info(dict(AEON_CFG, base_size=1 << 21))["total_anchors"] == 34596
    many = dict(AEON_CFG, height=16, width=16, ratios=[1.0] * 70, scales=[1.0] * 70)
    assert A.rcnn_config_info(many)["total_anchors"] == 4900 and len(A.rcnn_anchors(many)) == 4900
    with pytest.raises(A.AeonHipError) as e:  # 9 * 4000 * 4000 anchors: the table itself is refused
        A.rcnn_anchors(dict(AEON_CFG, height=64000, width=64000))
    assert e.value.code == A.AEON_HIP_EUNSUPPORTED


@pytest.fixture(scope="module")
def driver():
    assert os.path.exists("/opt/rocm/llvm/bin/clang++"), "no clang with sanitizer runtimes"
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "aeon_amd", "csrc"), "sanitize_rcnn"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")
    env.pop("LD_PRELOAD", None)

    def run(*args):
        r = subprocess.run([DRIVER] + list(args), capture_output=True, text=True, env=env, timeout=300)
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        return r
    return run


def test_shuffle_header_equals_std_shuffle(driver):
    r = driver("shuffle")
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    # 3 seeds x (301 + 3 sizes) x 4 prefix lengths, then 7 engine words
    assert r.stdout.strip() == "shuffle ok %d" % (3 * 304 * 4 + 7)


def test_host_code_runs_clean_under_sanitizers(driver):
    r = driver("sample")
    assert r.returncode == 0 and r.stdout.startswith("sample ok "), (r.stdout[-2000:], r.stderr[-2000:])
    cfgs = [AEON_CFG, dict(AEON_CFG, height=48, width=80, scales=[1, 2, 3]), dict(AEON_CFG, bogus=1),
            dict(AEON_CFG, ratios=[]), dict(AEON_CFG, scaling_factor=0), dict(AEON_CFG, height="x"),
            dict(AEON_CFG, ratios=[1e30], scales=[1e30]), dict(AEON_CFG, height=16, width=16, base_size=1)]
    r = driver("config", *[json.dumps(c) for c in cfgs], "{", "[]")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cfgs) + 2
    assert lines[0].startswith("ok 34596 128 (-84 -40 99 55) ") and lines[1].startswith("ok 135 ")
    assert all(l.startswith("error -1 ") for l in lines[2:6]), lines
    assert all(l.startswith("error ") for l in lines[8:]), lines
