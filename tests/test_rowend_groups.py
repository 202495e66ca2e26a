"""The hand-tuned chain's row ends since they run in groups of four positions (csrc/ntsc_decode_fast.hip: group_run; the
schedule: csrc/ntsc_rowend_plan.hpp): every width from 24 to 72 -- all residues mod 4 and mod 16 for every chroma delay,
rows narrower than the pipeline, 0 to 3 steady iterations, 0 to 4 encoder chunks, partial first and last groups -- the
benchmark's width with every row-end remainder, fields of one row, a wave that holds the end of one field and the start
of the next, and dropped and kept rows in one wave under head switching.  HIP == oracle/ntsc_oracle.c byte for byte
(tolerance 0: integer pixels in and out, fp64 filters in the reference's operation order), and the kernels that ran are
the hand-tuned ones, by name.

The composite -vhs forms with even scanline phases and the TV output filter (plain, wrap-around loads, pre-emphasis) take
the grouped row ends; the S-Video, any-phase (XA), full-output-filter (FO) and non-VHS forms keep the one-position row
ends and are held to the same widths.

Widths that are no multiple of four pixels reach the hand-tuned kernels through frames whose rows are padded to 16 bytes
(their precondition); the padding and the other field's rows must come back untouched."""
import numpy as np
import pytest

import _libs as L
import ntscsim

pytestmark = pytest.mark.gpu

FILL = 0x5A

FORMS = [
    ("vhs_sp", ["-vhs"], "k_encode_fast<double>", "k_decode_fast<true,double>"),
    ("vhs_lp", ["-vhs", "-vhs-speed", "lp"], "k_encode_fast<double>", "k_decode_fast<true,double>"),
    ("vhs_ep", ["-vhs", "-vhs-speed", "ep"], "k_encode_fast<double>", "k_decode_fast<true,double>"),
    ("vhs_svideo", ["-vhs", "-vhs-svideo", "1"], "k_encode_fast<double>", "k_decode_fast_sv<double>"),
    ("default", [], "k_encode_fast<double>", "k_decode_fast<false,double>"),
    ("xa", ["-vhs", "-comp-phase", "90"], "k_encode_fast_xi<double>", "k_decode_fast_xi<double>"),
    ("fo", ["-vhs", "-out-composite-lowpass-lite", "0"], "k_encode_fast<double>", "k_decode_fast_fo<double>"),
    ("pre", ["-vhs", "-comp-catv"], "k_encode_fast_pre<double>", "k_decode_fast_bk<true,double>"),
    ("pal_wrap", ["-tvstd", "pal", "-vhs"], "k_encode_fast<double>", "k_decode_fast<true,double,true>"),
]

# (width, height) sets, one test case per form and set so that each stays short
SIZES = {
    "w24_47": [(w, h) for w in range(24, 48) for h in (2, 5)],
    "w48_72": [(w, h) for w in range(48, 73) for h in (2, 5)],
    "bench_and_tall": [(w, 3) for w in range(717, 724)] + [(40, 130), (47, 130)],
}


def _run_case(sim, p, w, h, seed):
    """Two fields of one noise frame in ONE launch, each into a frame of its own.  Returns (got, expected, kernels)."""
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
    return out[:, :, :w], exp, sim.last_kernels()


def _chain(ran):
    return [k for k in ran if k.startswith(("k_encode", "k_decode", "k_vcr", "k_field_pipe"))]


@pytest.mark.parametrize("sizes", sorted(SIZES))
@pytest.mark.parametrize("name,flags,enc,dec", FORMS, ids=[f[0] for f in FORMS])
def test_row_ends_equal_the_oracle(name, flags, enc, dec, sizes):
    p = L.make_params(flags)
    sim = ntscsim.FieldSimulator(params=p)
    try:
        for (w, h) in SIZES[sizes]:
            got, exp, ran = _run_case(sim, p, w, h, 0x80E2D + 131 * w + h)
            bad = int((got != exp).sum())
            assert bad == 0, "%s %dx%d: %d mismatching bytes, first at %s" % (
                name, w, h, bad, tuple(int(i[0]) for i in np.nonzero(got != exp)))
            assert _chain(ran) == [enc, dec], (name, w, h, ran)
    finally:
        sim.close()


def _grey_rows(field_rows):
    """Rows whose every pixel has B == G == R: no chroma left (dropped), which a noise frame's kept rows never are."""
    px = field_rows.astype(np.int16)
    return ((px[..., 0] == px[..., 1]) & (px[..., 1] == px[..., 2])).all(axis=-1)


@pytest.mark.parametrize("w", [96, 97, 98, 99])
def test_dropped_and_kept_rows_share_a_wave_under_head_switching(w):
    """-chroma-dropout high enough that each field of 18 rows (one wave holds both) has rows with their chroma dropped
    beside rows that keep it, and a head-switching point that displaces the last rows beyond W / 10 samples."""
    h = 36
    p = L.make_params(["-vhs", "-chroma-dropout", "30000", "-vhs-head-switching-point", "0.105",
                       "-vhs-head-switching-phase", "0.002"])
    sim = ntscsim.FieldSimulator(params=p)
    try:
        got, exp, ran = _run_case(sim, p, w, h, 0xD20F + w)
        for k in range(2):
            rows = exp[k, ((k & 1) ^ 1)::2]                 # the rows this field wrote
            grey = _grey_rows(rows)
            assert grey.any() and not grey.all(), ("the oracle's field %d has no mix of dropped and kept rows" % k, grey)
        assert np.array_equal(got, exp)
        assert _chain(ran) == ["k_encode_fast<double>", "k_decode_fast<true,double,true>"], ran
    finally:
        sim.close()
