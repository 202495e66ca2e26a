"""The hand-tuned encoder / decoder at the sizes where a row leaves one loop for another: every width around the steady
loop's entry condition, every fill phase of the chroma delay (9, 12, 14 samples: SP, LP, EP), fields of one row, a halo
row with nothing above it, a wave that holds rows of two fields.  HIP == oracle/ntsc_oracle.c bit for bit (tolerance 0:
integer pixels in and out, fp64 filters in the reference's operation order), and the form that ran is the hand-tuned
one, by name.

Widths that are no multiple of four pixels reach the hand-tuned kernels through frames whose rows are padded to 16 bytes
(their precondition); the padding and the other field's rows must come back untouched."""
import numpy as np
import pytest

import _libs as L
import ntscsim

pytestmark = pytest.mark.gpu

# narrower than the pipeline is deep | the steady loop's entry condition and one either side | one and two steady
# iterations | the benchmark's width
WIDTHS = (16, 31, 39, 40, 41, 47, 64, 65, 720)
# one row per field (its halo row has no row above it) | a field of one row beside one of two | three rows | 65 rows per
# field: a wave of 63 rows + halo holds the end of one field and the start of the next
HEIGHTS = (2, 3, 5, 130)
FILL = 0x5A

FORMS = [
    ("vhs_sp", ["-vhs"], "k_encode_fast<double>", "k_decode_fast<true,double>"),
    ("vhs_lp", ["-vhs", "-vhs-speed", "lp"], "k_encode_fast<double>", "k_decode_fast<true,double>"),
    ("vhs_ep", ["-vhs", "-vhs-speed", "ep"], "k_encode_fast<double>", "k_decode_fast<true,double>"),
    ("vhs_svideo", ["-vhs", "-vhs-svideo", "1"], "k_encode_fast<double>", "k_decode_fast_sv<double>"),
    ("default", [], "k_encode_fast<double>", "k_decode_fast<false,double>"),
]


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


@pytest.mark.parametrize("name,flags,enc,dec", FORMS, ids=[f[0] for f in FORMS])
def test_row_edges_of_the_hand_tuned_chain_equal_the_oracle(name, flags, enc, dec):
    p = L.make_params(flags)
    sim = ntscsim.FieldSimulator(params=p)
    try:
        for w in WIDTHS:
            for h in HEIGHTS:
                got, exp, ran = _run_case(sim, p, w, h, 0x2D1E7 + 131 * w + h)
                bad = int((got != exp).sum())
                assert bad == 0, "%s %dx%d: %d mismatching bytes, first at %s" % (
                    name, w, h, bad, tuple(int(i[0]) for i in np.nonzero(got != exp)))
                chain = [k for k in ran if k.startswith(("k_encode", "k_decode", "k_vcr", "k_field_pipe"))]
                assert chain == [enc, dec], (name, w, h, ran)
    finally:
        sim.close()


@pytest.mark.parametrize("w,h", [(96, 36), (720, 5)])
def test_head_switch_beyond_a_tenth_of_the_row_takes_the_wrap_form(w, h):
    """PAL's default switching point displaces the last rows by more than W / 10 samples: the wrap-around loads."""
    p = L.make_params(["-tvstd", "pal", "-vhs"])
    sim = ntscsim.FieldSimulator(params=p)
    try:
        got, exp, ran = _run_case(sim, p, w, h, 0x51CE)
        assert np.array_equal(got, exp)
        assert [k for k in ran if k.startswith("k_decode")] == ["k_decode_fast<true,double,true>"], ran
    finally:
        sim.close()
