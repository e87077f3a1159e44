"""CPU: tiff_expand_large's code run on the host (tiff_gpu_emulate(..., large_strips=True)) against the pixels each file
of tests/tiff_large_cases.py was cut from, bit for bit, in the three modes; then the strips it must refuse."""
import pytest

import aeon_amd as A
from tests import test_tiff_tiles as T
from tests import tiff_large_cases as LC


def routed(name, f):  # only the opt-in call takes the file to the device: nothing below can pass without tiff_expand_large
    assert A.tiff_large_route(f) and not A.tiff_decoder_route(f), name


@pytest.mark.parametrize("k", range(LC.N_FILES))
def test_emulation_gives_the_source_pixels(k):
    assert len(LC.files()) == LC.N_FILES
    name, f, a, photo, event = LC.files()[k]
    routed(name, f)
    assert event is None or event(f), (name, "the writer's stream does not show what the case is for")
    for m in T.MODES:
        T.check(A.tiff_gpu_emulate(f, m, large_strips=True), a, photo, m, name)


@pytest.mark.parametrize("k", range(3))
def test_corrupt_large_strip_is_refused(k):
    name, f = LC.corrupt()[k]
    routed(name, f)
    with pytest.raises(A.AeonHipError) as e:
        A.tiff_gpu_emulate(f, large_strips=True)
    assert e.value.code == T.EDEVICE, name
    with pytest.raises(A.AeonHipError):  # the host decoder refuses it too
        A.decode_tiff(f)
