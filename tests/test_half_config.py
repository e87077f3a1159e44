"""CPU: float16 / bfloat16 image outputs on the host surface -- the numpy rounding the GPU tests
compare against, the image config's two new 'output_type' names (behind "extended_output_type": true, so
that no config changes its meaning), and every other ETL type still refusing them with the message it gives
for any unknown name."""
import numpy as np
import pytest

import aeon_amd as A
from aeon_amd import configs as C
from tests import half_ref as R


def _edge_floats():
    """Ties of both 16-bit types, float16 / bfloat16 subnormals, zeros of both signs, values at and
    above float16's 65504 (65520 is the tie that rounds to inf)."""
    bits = []
    for hi in (0x3F80, 0x3F81, 0x4000, 0x7F7E, 0x0001, 0x0000, 0x007F, 0x0080):  # bfloat16 ties and neighbours
        for lo in (0x7FFF, 0x8000, 0x8001, 0x0000, 0xFFFF):
            bits += [(hi << 16) | lo, 0x80000000 | (hi << 16) | lo]
    vals = np.array(bits, np.uint32).view(np.float32).tolist()
    vals += [0.0, -0.0, 65504.0, 65519.996, 65520.0, 65536.0, -65504.0, -65520.0, 1e6, -1e6, 3.0e38,
             2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0000001, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 5.96e-8, 6.1e-5,
             1.0 + 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, 1.0 + 3 * 2.0 ** -11, -1.0 - 2.0 ** -11]
    return np.array(vals, np.float32)


def test_bf16_helper_matches_torch():
    import torch
    rng = np.random.default_rng(16)
    x = np.concatenate([(rng.standard_normal(10000) * 10.0 ** rng.integers(-42, 38, 10000)).astype(np.float32), _edge_floats()])
    assert np.isfinite(x).all()
    want = torch.tensor(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.bf16_bits(x), want)
    # and float16 through numpy is the same IEEE rounding torch does
    want16 = torch.tensor(x).to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.f16_bits(x), want16)


def test_as_torch_views_without_copy():
    import torch
    x = _edge_floats()
    b = R.bf16_bits(x)
    t = A.as_torch(b, "bfloat16")
    assert t.dtype == torch.bfloat16 and t.data_ptr() == b.ctypes.data
    assert torch.equal(t, torch.tensor(x).to(torch.bfloat16))
    h = R.f16_bits(x).view(np.float16)
    t = A.as_torch(h, "float16")
    assert t.dtype == torch.float16 and t.data_ptr() == h.ctypes.data
    with pytest.raises(TypeError):
        A.as_torch(h, "bfloat16")


@pytest.mark.parametrize("name,code,npdt", [("float16", 7, np.float16), ("bfloat16", 8, np.uint16)])
@pytest.mark.parametrize("cn,major", [(3, True), (3, False), (1, True)])
def test_image_config_reports_half_types(name, code, npdt, cn, major):
    etl = {"type": "image", "height": 20, "width": 36, "channels": cn, "output_type": name, "channel_major": major,
           "extended_output_type": True}
    aug = {"type": "image", "mean": C.MEAN[:cn], "stddev": C.STDDEV[:cn]}
    d = A.Decoder(dict(batch_size=2, etl=[etl], augmentation=[aug]))
    (o,) = d.outputs
    assert o["type_name"] == name and o["dtype"] == npdt and A.DTYPES[name] == (code, npdt)
    assert o["item_bytes"] == 2 * cn * 20 * 36
    assert o["shape"] == ((cn, 20, 36) if major else (20, 36, cn))
    od = A.out_desc(channels=cn, dtype=name)
    assert od.dtype == code
    # the existing types say what they are too
    f = A.Decoder(dict(batch_size=2, etl=[dict(etl, output_type="float")], augmentation=[aug]))
    assert f.outputs[0]["type_name"] == "float32" and f.outputs[0]["dtype"] == np.float32


CLASSES = ["a", "b"]
OTHERS = {
    "pixelmask": {"type": "pixelmask", "height": 16, "width": 16, "channels": 1},
    "label": {"type": "label", "binary": False},
    "boundingbox": {"type": "boundingbox", "height": 32, "width": 32, "max_bbox_count": 4, "class_names": CLASSES},
    "video": {"type": "video", "max_frame_count": 2, "frame": {"height": 16, "width": 16}},
}


def _error_of(etl, aug):
    with pytest.raises(A.AeonHipError) as e:
        A.Decoder(dict(batch_size=2, etl=etl, augmentation=aug))
    return e.value.code, str(e.value)


@pytest.mark.parametrize("kind", sorted(OTHERS))
@pytest.mark.parametrize("name", ["float16", "bfloat16"])
def test_other_etl_types_refuse_half_as_before(kind, name):
    """The message of an unknown name ("float17") is the message of the half names."""
    img = {"type": "image", "height": 16, "width": 16, "channels": 3}
    aug = [{"type": "image"}]

    def etl(t):
        e = dict(OTHERS[kind])
        if kind == "video":
            e["frame"] = dict(e["frame"], output_type=t)
        else:
            e["output_type"] = t
        return [img, e] if kind in ("pixelmask", "label") else [e]
    code17, msg17 = _error_of(etl("float17"), aug)
    code, msg = _error_of(etl(name), aug)
    assert code == code17 and msg == msg17.replace("float17", name)
    assert code in (A.AEON_HIP_EINVAL, A.AEON_HIP_ERUNTIME)


@pytest.mark.parametrize("name", ["float16", "bfloat16"])
def test_fixed_aspect_ratio_refused(name):
    etl = {"type": "image", "height": 32, "width": 32, "channels": 3, "output_type": name, "extended_output_type": True}
    aug = {"type": "image", "fixed_aspect_ratio": True, "crop_enable": False}
    code, msg = _error_of([etl], [aug])
    assert code == A.AEON_HIP_EUNSUPPORTED and name in msg and "fixed_aspect_ratio" in msg
    # without the canvas the same config is fine, with and without standardization
    A.Decoder(dict(batch_size=2, etl=[etl], augmentation=[{"type": "image"}]))
    A.Decoder(dict(batch_size=2, etl=[etl], augmentation=[dict(C.C2_AUG)]))


def test_uint8_still_refuses_mean():
    etl = {"type": "image", "height": 32, "width": 32, "channels": 3, "output_type": "uint8_t"}
    code, msg = _error_of([etl], [dict(C.C2_AUG)])
    assert "supported only for float or double" in msg


@pytest.mark.parametrize("name", ["float16", "bfloat16"])
def test_image_without_the_key_refuses_as_before(name):
    """Without "extended_output_type": true (absent or false) an image config with a half name is what it was:
    invalid, with the message of any unknown name; the key with one of aeon's own types changes nothing; and
    no other element knows the key."""
    etl = {"type": "image", "height": 32, "width": 32, "channels": 3}
    aug = [{"type": "image"}]
    code17, msg17 = _error_of([dict(etl, output_type="float17")], aug)
    for extra in ({}, {"extended_output_type": False}):
        code, msg = _error_of([dict(etl, output_type=name, **extra)], aug)
        assert (code, msg) == (code17, msg17)
    code, msg = _error_of([dict(etl, output_type="float17", extended_output_type=True)], aug)
    assert (code, msg) == (code17, msg17)
    d = A.Decoder(dict(batch_size=2, etl=[dict(etl, output_type="float", extended_output_type=True)], augmentation=aug))
    assert d.outputs[0]["type_name"] == "float32"
    code, msg = _error_of([etl, dict(OTHERS["pixelmask"], extended_output_type=True)], aug)
    assert code in (A.AEON_HIP_EINVAL, A.AEON_HIP_ERUNTIME) and "extended_output_type" in msg
