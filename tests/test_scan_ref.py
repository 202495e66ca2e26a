"""The scanimate checker tests/_scan_ref.py against fields recorded from the reference's own lines
(tests/golden/scan_ref.npz: ffmpeg_scanimate.cpp:817-974 compiled behind a stand-in AVFrame, destination zeroed as
the tool's memset :1196 leaves it), byte for byte, and the vectorised checker against its scalar form.  No GPU."""
import os

import numpy as np
import pytest

import _scan_ref as R

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scan_ref.npz"))
NAMES = [str(n) for n in GOLDEN["names"]]
FIELDNOS = [int(f) for f in GOLDEN["fieldnos"]]


def test_golden_covers_the_effects_and_both_parities():
    assert FIELDNOS == [0, 45, 179, 181, 269, 270, 359, 361, 500, 541, 585, 700]
    assert set(R.effect_of(f)[0] for f in FIELDNOS) == {0, 1, 2, 3}
    assert set(R.field_of(f) for f in FIELDNOS) == {0, 1}
    assert [tuple(int(v) for v in GOLDEN[n + "_geom"]) for n in NAMES] == [(24, 40, 36, 24, 0), (24, 24, 36, 24, 1), (20, 16, 64, 48, 1)]


@pytest.mark.parametrize("name", NAMES)
def test_checker_reproduces_the_reference(name):
    sw, sh, dw, dh, inntsc = (int(v) for v in GOLDEN[name + "_geom"])
    src, want = GOLDEN[name + "_src"], GOLDEN[name + "_out"]
    assert src.shape == (sh, sw, 4) and want.shape == (len(FIELDNOS), dh, dw, 4)
    lit = 0
    for i, fieldno in enumerate(FIELDNOS):
        acc, got = R.scan_field(src, dw, dh, inntsc, fieldno)
        assert int((got != want[i]).sum()) == 0, "%s field %d" % (name, fieldno)
        assert int((np.minimum(acc >> 1, 255) != want[i][..., 0])[R.field_of(fieldno):].sum()) == 0
        if fieldno == 270:                                                       # |1 - 2 * 90 / 180| = 0: no signal at all
            assert int(acc.max()) == 0 and int(want[i][..., :3].max()) == 0
        lit += int((want[i][..., 0] > 0).sum())
    assert lit > 0


def test_scalar_and_vectorised_checker_agree():
    name = NAMES[1]                                                              # the smallest: 24 x 24 -> 36 x 24
    sw, sh, dw, dh, inntsc = (int(v) for v in GOLDEN[name + "_geom"])
    src = GOLDEN[name + "_src"]
    for fieldno in (0, 181, 361, 585, 700):
        a0, f0 = R.scan_field(src, dw, dh, inntsc, fieldno)
        a1, f1 = R.scan_field_scalar(src, dw, dh, inntsc, fieldno)
        assert int((a0 != a1).sum()) == 0 and int((f0 != f1).sum()) == 0, fieldno
    mono = GOLDEN[NAMES[0] + "_src"]
    a0, f0 = R.scan_field(mono, 36, 24, 0, 45)
    a1, f1 = R.scan_field_scalar(mono, 36, 24, 0, 45)
    assert int((a0 != a1).sum()) == 0 and int((f0 != f1).sum()) == 0


def test_effect_numbering_in_the_tools_types():
    assert [R.effect_of(f) for f in (0, 179, 180, 719, 720)] == [(0, 0), (0, 179), (1, 0), (3, 179), (0, 0)]
    assert R.effect_of((1 << 32) + 5) == (1, 81)                                 # (2^32 + 5) // 180 = 23860929, odd
