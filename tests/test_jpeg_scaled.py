"""CPU: the geometry of a JPEG file decoded at 1/2, 1/4, 1/8 (aeon_jpeg_scaled_plan, no device) against libjpeg's
rule restated here, and the refusals of the scaled call."""
import numpy as np
import pytest

import aeon_amd as A
from tests import jpeg_blocks as JB
from tests import jpeg_size_cases as J

LAYOUTS = ("gray", "s444", "s420", "s422", "s440", "s411")
SIZES = ((8, 8), (9, 17), (35, 50), (129, 70), (4, 61))  # (4 wide: two chroma samples a row, no fancy filter)


def jpg(layout, w, h):
    name = f"scaled_{layout}_{w}x{h}"
    return JB.gray(name, w, h) if layout == "gray" else JB.ycc(name, w, h, J.YCC[layout])


def rule(w, h, samp, s):
    """jdmaster.c jpeg_core_output_dimensions and jdsample.c jinit_upsampler: (n, dw, dh, upsampler) per component."""
    hmax, vmax, mn, out = max(c[0] for c in samp), max(c[1] for c in samp), 8 // s, []
    for hs, vs in samp:
        n = mn
        while n < 8 and (hmax * mn) % (hs * n * 2) == 0 and (vmax * mn) % (vs * n * 2) == 0:
            n *= 2
        dw, dh = -(-w * hs * n // (hmax * 8)), -(-h * vs * n // (vmax * 8))
        hf, vf = hmax * mn // (hs * n), vmax * mn // (vs * n)
        up = J.upsample_mode(hf, vf, dw)
        out.append((n, dw, dh, J.UP_BOX if mn == 1 and up != J.UP_FULL else up))
    return out


@pytest.mark.parametrize("scale", [1, 2, 4, 8])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_plan_follows_the_rule(layout, scale):
    for w, h in SIZES:
        data, samp = jpg(layout, w, h), J.SAMP[layout]
        d = A.ImgDesc(offset=0, width=-(-w // scale), height=-(-h // scale), stride=-(-w // scale) * 3, channels=3)
        plan = A.jpeg_scaled_plan(data, scale, 3, d)
        assert plan == rule(w, h, samp, scale), (w, h)
        assert plan[0][:3] == (8 // scale, d.width, d.height)  # luma: the record's own grid
        if scale == 1:
            assert plan == [(8, c.dw, c.dh, c.up) for c in J.components(w, h, samp)]
        if len(samp) == 3:  # a gray record of a YCbCr file needs the luma alone
            assert A.jpeg_scaled_plan(data, scale, 1) == [plan[0], (0, 0, 0, 0), (0, 0, 0, 0)]


def test_plan_consequences():
    """What the rule comes to: 4:2:0 chroma at twice the luma's IDCT size and no upsampling; 4:2:2 / 4:4:0 fancy at
    scales 2 and 4, box at 8; 4:1:1 box throughout."""
    ups = lambda layout, s: [c[3] for c in A.jpeg_scaled_plan(jpg(layout, 35, 50), s)]
    for s in (2, 4, 8):
        assert [c[0] for c in A.jpeg_scaled_plan(jpg("s420", 35, 50), s)] == [8 // s, 16 // s, 16 // s]
        assert ups("s420", s) == [J.UP_FULL] * 3 and ups("s411", s)[1:] == [J.UP_BOX] * 2
        assert ups("s422", s)[1] == (J.UP_BOX if s == 8 else J.UP_H2V1)
        assert ups("s440", s)[1] == (J.UP_BOX if s == 8 else J.UP_H1V2)


@pytest.mark.parametrize("scale,size,text,code", [
    (3, None, "scale 3 is not 1, 2, 4 or 8", A.AEON_HIP_EINVAL),
    (0, None, "scale 0 is not 1, 2, 4 or 8", A.AEON_HIP_EINVAL),
    (2, (17, 25), "decoded size 18x25 at scale 2 does not match the record descriptor 17x25", A.AEON_HIP_EINVAL),
    (8, (35, 50), "decoded size 5x7 at scale 8 does not match", A.AEON_HIP_EINVAL)])
def test_refusals(scale, size, text, code):
    d = size and A.ImgDesc(offset=0, width=size[0], height=size[1], stride=size[0] * 3, channels=3)
    with pytest.raises(A.AeonHipError, match=text + r".* \(record 0\)") as e:
        A.jpeg_scaled_plan(jpg("s420", 35, 50), scale, 3, d)
    assert e.value.code == code


def test_four_components_are_refused_above_scale_1():
    data = JB.four("scaled_cmyk", 35, 50, *J.FOUR["cmyk_22"])
    assert [c[0] for c in A.jpeg_scaled_plan(data, 1)] == [8] * 4
    with pytest.raises(A.AeonHipError, match=r"four-component .* not at scale 4 \(record 0\)") as e:
        A.jpeg_scaled_plan(data, 4)
    assert e.value.code == A.AEON_HIP_EUNSUPPORTED


@pytest.mark.parametrize("scale", [True, [2, np.True_]])
def test_a_bool_is_no_scale(scale):
    with pytest.raises(TypeError, match="not a bool"):  # (before the context is touched)
        A.Context.decode_jpeg_batch(None, [jpg("s420", 35, 50)] * 2, [A.ImgDesc()] * 2, 0, scale=scale)


@pytest.mark.parametrize("kw", [dict(regions=[None]), dict(progressive=True)])
def test_scale_goes_with_neither_regions_nor_progressive(kw):
    with pytest.raises(ValueError, match="scale alone"):  # (before the context is touched)
        A.Context.decode_jpeg_batch(None, [jpg("s420", 35, 50)], [], 0, scale=2, **kw)
