"""The mode model (oracle/ntsc_modes_oracle.c) on the CPU.

exact64 -- the model with every quantisation kept and the oracle's poles -- must BE the pinned oracle: same bytes, same taps,
same number of draws, over the switch sets of tests/cases.py and a few tiny / odd geometries.  That ties the model's
structure (delays, raw tails, zero fill, head-switch remap, field parity, draw order) to the oracle; the flavours that
define the tolerance modes differ from it only in what the named quantising operations and the poles do.
"""
import numpy as np
import pytest

import _libs as L
import _modes as M
from cases import CASES, case_jobs, make_source

TAPS = [n for n, _ in L.OracleTaps._fields_]

# tiny and odd geometries on top of the matrix: rows shorter than every filter delay, one-row fields, odd sizes
TINY = [
    ("tiny_vhs_5x3", ["-vhs"], 5, 3, 3, "noise", 0, 0),
    ("tiny_vhs_2x2", ["-vhs"], 2, 2, 2, "noise", 0, 0),
    ("tiny_ep_13x5", ["-vhs", "-vhs-speed", "ep"], 13, 5, 3, "noise", 0, 0),
    ("tiny_def_3x1", [], 3, 1, 2, "noise", 0, 0),
    ("tiny_def_7x9", [], 7, 9, 2, "noise", 1, 1),
    ("tiny_vhs_pal_21x7", ["-tvstd", "pal", "-vhs", "-vhs-head-switching-point", "0.085"], 21, 7, 4, "noise", 0, 0),
    ("tiny_ghost", ["-vhs"], 24, 6, 2, "noise", 0, 0),
]


def _params(name, flags):
    p = L.make_params(flags)
    if name == "tiny_ghost":
        p.ghost_taps = 2
        p.ghost_delay[0], p.ghost_gain[0] = 3, 64
        p.ghost_delay[1], p.ghost_gain[1] = 11, -32
    return p


@pytest.mark.parametrize("case", CASES + TINY, ids=[c[0] for c in CASES + TINY])
def test_exact64_is_the_oracle(case):
    name, flags, w, h, n, kind, il, tff = case
    p = _params(name, flags)
    srcs = [make_source(kind, w, h, j) if kind != "noise" else L.noise_frame(w, h, 0x1234567 + j) for j in range((n + 1) // 2)]
    o, m = L.OracleStream(p), M.ModelStream(p, "exact64")
    for si, field, fieldno in case_jobs(n):
        a = np.full((h, w, 4), 0x5A, np.uint8)
        b = np.full((h, w, 4), 0x5A, np.uint8)
        ta = o.field(a, srcs[si], field, fieldno, il, tff, taps=TAPS)
        tb = m.field(b, srcs[si], field, fieldno, il, tff, taps=TAPS)
        assert m.rng_pos == o.rng_pos, (name, fieldno)
        for t in TAPS:
            assert np.array_equal(ta[t], tb[t]), (name, fieldno, t)
        assert a.tobytes() == b.tobytes(), (name, fieldno)


@pytest.mark.parametrize("case", [c for c in CASES if c[2] * c[3] <= 4096][::3] + TINY[:3], ids=lambda c: c[0])
def test_fast32_runs_and_draws_like_the_oracle(case):
    name, flags, w, h, n, kind, il, tff = case
    p = _params(name, flags)
    src = L.noise_frame(w, h, 9)
    o, m = L.OracleStream(p), M.ModelStream(p, "fast32")
    for si, field, fieldno in case_jobs(n):
        a = np.zeros((h, w, 4), np.uint8)
        b = np.full((h, w, 4), 0x5A, np.uint8)
        o.field(a, src, field, fieldno, il, tff)
        m.field(b, src, field, fieldno, il, tff)
        assert m.rng_pos == o.rng_pos
        assert (b[1 - field::2] == 0x5A).all() and not b[field::2, :, 3].any()
        # float filters in place of double ones: a unit of the 256-scaled signal here and there, never a whole step more
        assert np.abs(a[field::2].astype(np.int16) - b[field::2].astype(np.int16)).max() <= 1


@pytest.mark.parametrize("case", [c for c in M.FLOAT_CASES if c[2] * c[3] <= 8192], ids=lambda c: c[0])
def test_real64_draws_and_rows(case):
    """real64 consumes exactly the oracle's draws, leaves the other field's rows alone, writes alpha 0 and the byte of
    every channel is clamp(trunc(v)) of the value it reports"""
    name, flags, w, h, n, kind, form, extra = case
    p = L.make_params(flags)
    srcs = M.sources(kind, w, h)
    il, tff = extra.get("interlaced", 0), extra.get("tff", 0)
    o, m = L.OracleStream(p), M.ModelStream(p, "real64")
    for si, field, fieldno in M.jobs(min(n, 4), len(srcs)):
        a = np.zeros((h, w, 4), np.uint8)
        b = np.full((h, w, 4), 0x5A, np.uint8)
        o.field(a, srcs[si], field, fieldno, il, tff)
        out = m.field(b, srcs[si], field, fieldno, il, tff)
        assert m.rng_pos == o.rng_pos, (name, fieldno)
        assert (b[1 - field::2] == 0x5A).all()
        assert not b[field::2, :, 3].any()
        q = np.clip(np.trunc(out["v"]), 0, 255).astype(np.uint8)
        assert np.array_equal(b[field::2, :, 2::-1], q)          # memory order B, G, R
        # the definition stays within the mode's stated +-1 LSB of the truncating oracle
        assert np.abs(a[field::2].astype(np.int16) - b[field::2].astype(np.int16)).max() <= 1


NOISE_OFF = ["-noise", "0", "-chroma-noise", "0", "-chroma-phase-noise", "0", "-chroma-dropout", "0"]


@pytest.mark.parametrize("flags", [NOISE_OFF, ["-vhs", "-vhs-head-switching", "0"] + NOISE_OFF,
                                   ["-vhs", "-vhs-speed", "ep", "-vhs-head-switching", "0"] + NOISE_OFF],
                         ids=["default", "vhs", "vhs_ep"])
def test_real64_reproduces_flat_grey(flags):
    """One flat mid-grey, all noise off: nothing in the chain but filters with unit DC gain, so away from the row ends the
    value in front of the truncation IS the grey -- plus the luma constant, which is negative (it takes back the half
    units that the dropped truncations no longer take): grey + bias / 256, below the grey."""
    w, h, grey = 720, 6, 128
    p = L.make_params(flags)
    src = np.zeros((h, w, 4), np.uint8)
    src[..., :3] = grey
    interior = slice(500, 650)          # (the 280 kHz chroma poles of EP have settled to 1e-9 by then)
    for bias in (0.0, M.luma_bias(p)):
        m = M.ModelStream(p, "real64")
        dst = np.zeros((h, w, 4), np.uint8)
        out = m.field(dst, src, 1, 0, bias=bias)
        assert m.rng_pos == 0
        v = out["v"][:, interior]
        assert np.abs(v - (grey + bias / 256.0)).max() < 1e-6, np.abs(v - (grey + bias / 256.0)).max()
        assert np.abs(out["final_i"][:, interior]).max() < 1e-6 and np.abs(out["final_q"][:, interior]).max() < 1e-6
    assert bias < 0 and (out["v"][:, interior] < grey).all()
    # and half a step up the truncation gives the grey back: the byte of (grey + 0.5) is the grey, with either constant
    m = M.ModelStream(p, "real64")
    dst = np.zeros((h, w, 4), np.uint8)
    m.field(dst, src, 1, 0, bias=128.0 + M.luma_bias(p))
    assert (dst[1::2, interior, :3] == grey).all()


def test_real32_is_close_to_real64():
    """the fp32 evaluation of the definition: same draws, values within a small fraction of 1/256 of a step"""
    w, h = 68, 10
    p = L.make_params(["-vhs"])
    src = L.noise_frame(w, h, 77)
    a, b = M.ModelStream(p, "real64"), M.ModelStream(p, "real32")
    da, db = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 4), np.uint8)
    oa, ob = a.field(da, src, 1, 0), b.field(db, src, 1, 0)
    assert a.rng_pos == b.rng_pos
    assert np.abs(oa["v"] - ob["v"]).max() < 1.0 / 64
    assert np.abs(oa["composite"] - ob["composite"]).max() < 0.25
