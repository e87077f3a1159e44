"""CPU: the block rectangles of a JPEG region decode (aeon_jpeg_region_plan) against the rule restated here (the
samples under the region, one more each side along a row for h2v1 / h2v2 and down a column for h1v2 / h2v2, clipped,
then the blocks covering them), and the decode call's refusals, which the plan entry makes with the same code."""
import pytest

import aeon_amd as A
from tests import jpeg_blocks as JB
from tests import jpeg_size_cases as J

# (layout, width, height): between them every upsampler -- full (s444, every luma), h2v1 (s422), h1v2 (s440), h2v2
# (s420), box (s411's chroma by 4; the chroma of a 4:2:0 file 4 wide)
FILES = [("s444", 75, 61), ("s422", 75, 61), ("s440", 75, 61), ("s420", 75, 61), ("s411", 75, 61), ("s420", 4, 61)]


def regions(w, h):
    """Both image edges, one sample short of them, the interior (odd and block-aligned), single rows and columns."""
    r = [(0, 0, 1, 1), (w - 1, h - 1, 1, 1), (w - 1, 0, 1, 1), (0, h - 1, 1, 1), (1, 1, w - 2, h - 2),
         (0, h // 2, w, 1), (w // 2, 0, 1, h), (0, 0, w, h - 1), (0, 0, w - 1, h)]
    if w > 48:
        r += [(17, 9, 30, 21), (16, 16, 16, 16), (15, 15, 2, 2), (32, 31, 43, 30)]
    return r


def rule(c, x, y, w, h):
    nx, ny = c.up in (J.UP_H2V1, J.UP_H2V2), c.up in (J.UP_H1V2, J.UP_H2V2)
    x0, x1 = max(x // c.hf - nx, 0), min((x + w - 1) // c.hf + nx, c.dw - 1)
    y0, y1 = max(y // c.vf - ny, 0), min((y + h - 1) // c.vf + ny, c.dh - 1)
    return (x0 // 8, y0 // 8, x1 // 8 - x0 // 8 + 1, y1 // 8 - y0 // 8 + 1)


@pytest.mark.parametrize("layout,w,h", FILES)
def test_plan_follows_the_rule(layout, w, h):
    data = JB.ycc(f"region_{layout}_{w}x{h}", w, h, J.YCC[layout])
    comps = J.components(w, h, J.YCC[layout])
    assert A.jpeg_region_plan(data) == [(0, 0, c.bw, c.bh) for c in comps]  # the whole image: the frame's grid
    assert A.jpeg_region_plan(data, (0, 0, w, h)) == A.jpeg_region_plan(data)
    for r in regions(w, h):
        assert A.jpeg_region_plan(data, r) == [rule(c, *r) for c in comps], r
        # a gray record of a colour file reads the luma plane alone
        assert A.jpeg_region_plan(data, r, channels=1) == [rule(comps[0], *r), (0,) * 4, (0,) * 4], r


@pytest.mark.parametrize("region,desc,text", [
    ((3, 3, 0, 5), None, r"JPEG: region \(3, 3, 0, 5\) is empty"),
    ((3, 3, 5, -1), None, r"JPEG: region \(3, 3, 5, -1\) is empty"),
    ((70, 0, 6, 5), None, r"JPEG: region \(70, 0, 6, 5\) reaches outside the 75x61 image"),
    ((0, 57, 5, 5), None, r"JPEG: region \(0, 57, 5, 5\) reaches outside"),
    ((-1, 0, 5, 5), None, r"JPEG: region \(-1, 0, 5, 5\) reaches outside"),
    ((8, 8, 9, 5), (9, 6), r"JPEG: record descriptor 9x6 is not the size of region \(8, 8, 9, 5\)"),
    ((0, 0, 75, 61), (75, 60), r"JPEG: decoded size 75x61 does not match the record descriptor 75x60"),
])
def test_refusals(region, desc, text):
    data = JB.ycc("region_s420_75x61", 75, 61, J.YCC["s420"])
    d = desc and A.ImgDesc(offset=0, width=desc[0], height=desc[1], stride=desc[0] * 3, channels=3)
    with pytest.raises(A.AeonHipError, match=text + r".* \(record 0\)") as e:
        A.jpeg_region_plan(data, region, desc=d)
    assert e.value.code == A.AEON_HIP_EINVAL
