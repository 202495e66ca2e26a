"""The luma delay ring of the hand-tuned -vhs decoder (csrc/ntsc_decode_fast.hip: luma_take; csrc/ntsc_rowend_plan.hpp:
luma_ring).  At tape speed SP the grouped rows of the composite -vhs forms no longer load and box-filter the composite
samples a second time for the VCR's luma path: the first separator's box value waits 14 positions in a 16-slot LDS ring.
What can go wrong is the ring's bookkeeping -- which slot a position lands in as the ring wraps, what a read finds before
the row's first sample and behind its last one (zeros enter the box from the left at the fill, from the right at the
drain, and from either side under head switching), and whether a launch that must not run the ring (LP, EP: LOFF = 17 / 19
do not fit 16 slots) really keeps the re-read -- so:

  * widths 40 to 96 at heights 2 and 5: 3 to 17 steady iterations between fill and drain (SP), the ring wraps 4 to 7
    times over the row's W + 24 positions, every residue mod 4 and mod 16, partial first and last groups; widths 24
    to 39 besides, across the narrowest row that takes the groups and with them the ring (width 30: one steady
    iteration; below it the one-position path and no ring); the forms -vhs (SP), -vhs -comp-catv (pre-emphasis: BK)
    and -tvstd pal -vhs (wrap-around loads: WR), and -vhs-speed lp / ep, which must stay on the re-read path;
  * head switching with small and large displacements of either sign beside undisplaced rows in one wave (the reference
    gives a field ONE sign -- the displacement decays by 7/8 per row -- so the two signs are separate cases, each with
    its zero-displacement rows before the switch point and after the decay);
  * one case at width 720, one of 130 rows (a wave holds the end of one field and the start of the next).

EXACT mode: HIP == oracle/ntsc_oracle.c byte for byte (tolerance 0), rng_pos equal, padding and the other field's rows
untouched; that also shows the drain needs no special case (the separator's zero pushes ARE the box's tail).  FAST32 mode
(float filter states; the ring holds integers, so the ring form computes what the re-read form computed): the stated
tolerance of tests/test_gpu_fast_mode.py, +-1 LSB per channel and at most 1 % of the pixels different -- the fraction
taken over all pixels of a case's sweep, since one pixel of a 40 x 1 field is already 2.5 %.  The kernels that ran are
asserted by name, and the path by the decoder launch's dynamic LDS (ntscsim_debug_last_decoder_lds): 4096 bytes with
the ring, 0 without."""
import math

import numpy as np
import pytest

import _libs as L
import ntscsim
from ntscsim import _capi

pytestmark = pytest.mark.gpu

FILL = 0x5A
RING_BYTES = 16 * 64 * 4

# name, switches, chroma delay, encoder, decoder (RT = double / float is filled in)
FORMS = [
    ("vhs_sp", ["-vhs"], 9, "k_encode_fast<%s>", "k_decode_fast<true,%s>"),
    ("pre", ["-vhs", "-comp-catv"], 9, "k_encode_fast_pre<%s>", "k_decode_fast_bk<true,%s>"),
    ("pal_wrap", ["-tvstd", "pal", "-vhs"], 9, "k_encode_fast<%s>", "k_decode_fast<true,%s,true>"),
    ("vhs_lp", ["-vhs", "-vhs-speed", "lp"], 12, "k_encode_fast<%s>", "k_decode_fast<true,%s>"),
    ("vhs_ep", ["-vhs", "-vhs-speed", "ep"], 14, "k_encode_fast<%s>", "k_decode_fast<true,%s>"),
]

SIZES = {
    "w24_39": [(w, h) for w in range(24, 40) for h in (2, 5)],      # across the threshold: the ring runs from width 30
    "w40_58": [(w, h) for w in range(40, 59) for h in (2, 5)],
    "w59_77": [(w, h) for w in range(59, 78) for h in (2, 5)],
    "w78_96": [(w, h) for w in range(78, 97) for h in (2, 5)],
    "wide_and_tall": [(720, 3), (41, 130), (64, 130)],
}


def _ring_bytes(w, d):
    """rowend::luma_ring: SP only (LOFF = 5 + d = 14), and only rows the steady loop enters (the grouped ones)."""
    skt = 15 + d
    t_end = w - (d - 7 if d > 7 else 0)
    return RING_BYTES if (d == 9 and t_end - skt >= 4) else 0


def _run_case(sim, p, w, h, seed):
    """Two fields of one noise frame in ONE launch, each into a frame of its own (tests/test_rowend_groups.py).
    Returns (got, expected, kernels, decoder LDS)."""
    import torch
    wp = (w + 3) & ~3
    frame = L.noise_frame(w, h, seed)
    o = L.OracleStream(p)
    exp = np.full((2, h, w, 4), FILL, np.uint8)
    jobs = [(0, k, (k & 1) ^ 1, k) for k in range(2)]
    for (si, di, field, fieldno) in jobs:
        o.field(exp[di], frame, field, fieldno)
    src_p = np.zeros((1, h, wp, 4), np.uint8)
    src_p[0, :, :w] = frame
    src = torch.from_numpy(src_p).cuda()
    dst = torch.full((2, h, wp, 4), FILL, dtype=torch.uint8, device="cuda")
    sim.rng_pos = 0
    sim.fields(src[:, :, :w], dst[:, :, :w], jobs)
    sim.sync()
    out = dst.cpu().numpy()
    assert (out[:, :, w:] == FILL).all(), "padding bytes were written (%dx%d)" % (w, h)
    assert sim.rng_pos == o.rng_pos
    return out[:, :, :w], exp, sim.last_kernels(), sim.last_decoder_lds()


def _chain(ran):
    return [k for k in ran if k.startswith(("k_encode", "k_decode", "k_vcr", "k_field_pipe"))]


@pytest.mark.parametrize("sizes", sorted(SIZES))
@pytest.mark.parametrize("name,flags,d,enc,dec", FORMS, ids=[f[0] for f in FORMS])
def test_exact_equals_the_oracle(name, flags, d, enc, dec, sizes):
    p = L.make_params(flags)
    sim = ntscsim.FieldSimulator(params=p)
    try:
        for (w, h) in SIZES[sizes]:
            got, exp, ran, lds = _run_case(sim, p, w, h, 0x10AA + 131 * w + h)
            bad = int((got != exp).sum())
            assert bad == 0, "%s %dx%d: %d mismatching bytes, first at %s" % (
                name, w, h, bad, tuple(int(i[0]) for i in np.nonzero(got != exp)))
            assert _chain(ran) == [enc % "double", dec % "double"], (name, w, h, ran)
            assert lds == _ring_bytes(w, d), (name, w, h, lds)
    finally:
        sim.close()


@pytest.mark.parametrize("sizes", sorted(SIZES))
@pytest.mark.parametrize("name,flags,d,enc,dec", FORMS[:3], ids=[f[0] for f in FORMS[:3]])
def test_fast32_within_stated_tolerance(name, flags, d, enc, dec, sizes):
    p = L.make_params(flags)
    sim = ntscsim.FieldSimulator(params=p)
    sim.set_mode(_capi.MODE_FAST32)
    pixels = different = 0
    try:
        for (w, h) in SIZES[sizes]:
            got, exp, ran, lds = _run_case(sim, p, w, h, 0x32AA + 131 * w + h)
            diff = np.abs(got.astype(np.int16) - exp.astype(np.int16))
            assert diff.max() <= 1, (name, w, h, int(diff.max()))
            for k in range(2):
                field = (k & 1) ^ 1
                assert (got[k][1 - field::2] == FILL).all(), (name, w, h, "other field's rows written")
                assert not got[k][field::2, :, 3].any()
                pixels += diff[k][field::2].shape[0] * w
                different += int((diff[k][field::2].max(axis=-1) > 0).sum())
            assert _chain(ran) == [enc % "float", dec % "float"], (name, w, h, ran)
            assert lds == _ring_bytes(w, d), (name, w, h, lds)
        assert different <= 0.01 * pixels, (name, sizes, different, pixels)
    finally:
        sim.close()


def _head_switch_rows(w, h, point, phase, field):
    """The displacement of every row of one NTSC field without phase noise (ffmpeg_ntsc.cpp:1660-1697)."""
    tw = w + w // 10
    t = tw * 262.5
    y = (int((point - math.trunc(point)) * t) // tw) * 2 + field - (262 - 240) * 2
    hx = int((phase - math.trunc(phase)) * t) % tw
    ishif = hx - tw if hx >= tw // 2 else hx
    rows, shif, shy = {}, 0, 0
    while y < h:
        if y >= 0:
            rows[y] = shif
        shif = ishif if shy == 0 else int(shif * 7 / 8)
        y += 2
        shy += 1
    return [rows.get(y, 0) for y in range(field, h, 2)]


# the displaced column hx of the switch: +8 / -8 (within W / 10: the plain form), just below / above half the 1.1 W window
# (the largest displacements of either sign: the wrap-around form)
HS = [("small_pos", lambda tw: 8, 1, "k_decode_fast<true,double>"),
      ("small_neg", lambda tw: tw - 8, -1, "k_decode_fast<true,double>"),
      ("large_pos", lambda tw: tw // 2 - 3, 1, "k_decode_fast<true,double,true>"),
      ("large_neg", lambda tw: tw // 2 + 3, -1, "k_decode_fast<true,double,true>")]


@pytest.mark.parametrize("w", [96, 99])
@pytest.mark.parametrize("name,hx,sign,dec", HS, ids=[c[0] for c in HS])
def test_zeros_enter_the_box_from_both_sides_under_head_switching(name, hx, sign, dec, w):
    """Two fields of 18 rows in one wave; the switch point leaves the first rows of each undisplaced, the displacement
    then decays to zero again: displaced and undisplaced rows side by side in the lanes of one wave.  A positive
    displacement reads zeros behind the row's right end (they enter the ring through the steady loop's loads), a negative
    one before its left end."""
    h = 36
    tw = w + w // 10
    point = "0.105"
    phase = "%.8f" % ((hx(tw) + 0.5) / (tw * 262.5))
    for field in (0, 1):
        rows = _head_switch_rows(w, h, float(point), float(phase), field)
        moved = [s for s in rows if s]
        assert moved and all((s > 0) == (sign > 0) for s in moved) and rows.count(0) >= 2, (name, rows)
        assert (max(abs(s) for s in moved) <= w // 10) == name.startswith("small"), (name, rows)
    p = L.make_params(["-vhs", "-vhs-head-switching-point", point, "-vhs-head-switching-phase", phase])
    sim = ntscsim.FieldSimulator(params=p)
    try:
        got, exp, ran, lds = _run_case(sim, p, w, h, 0x45D0 + w)
        assert np.array_equal(got, exp), (name, w, int((got != exp).sum()))
        assert _chain(ran) == ["k_encode_fast<double>", dec], ran
        assert lds == RING_BYTES
    finally:
        sim.close()
