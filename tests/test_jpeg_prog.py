"""CPU: the progressive path's host half and its device code run on the host (aeon_jpeg_prog_route,
aeon_jpeg_prog_emulate: jpeg_prog.hpp's wave logic, one unit after another) over tests/jpeg_prog_cases.py, against the
host entropy decoder's sparse stream (aeon_jpeg_entropy_decode) -- the whole tuple, the stream's hash included."""
import numpy as np
import pytest

import aeon_amd as A
from tests import jpeg_prog_cases as PC

NAMES = sorted(PC.files())


@pytest.mark.parametrize("name", NAMES)
def test_routed_and_equal_to_the_host_decoder(name):
    f = PC.files()[name]
    assert A.jpeg_prog_route(f), name
    assert A.jpeg_prog_emulate(f) == A.jpeg_entropy_decode(f), name


def test_no_code_for_sixteen_ones():
    bad = PC.corrupt()
    assert A.jpeg_prog_route(bad)
    with pytest.raises(A.AeonHipError):
        A.jpeg_entropy_decode(bad)
    with pytest.raises(A.AeonHipError) as e:
        A.jpeg_prog_emulate(bad)
    assert "JPEG" in str(e.value)


def test_cut_off_mid_scan_reads_zeros_as_the_host_does():
    f = PC.cut()
    assert A.jpeg_prog_route(f) and len(f) < len(PC.files()["s444_64x64_q100"])
    assert A.jpeg_prog_emulate(f) == A.jpeg_entropy_decode(f)
    assert A.jpeg_prog_emulate(f) != A.jpeg_entropy_decode(PC.files()["s444_64x64_q100"])


def test_sequential_files_keep_their_route():
    z = np.load(PC.GOLDEN + "/jpeg_fixtures.npz")
    for k in ("s420_q50.jpg", "s444_rst.jpg", "gray_q70.jpg"):
        assert not A.jpeg_prog_route(z[k].tobytes()), k
        with pytest.raises(A.AeonHipError):
            A.jpeg_prog_emulate(z[k].tobytes())
