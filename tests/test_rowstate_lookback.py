"""The row-start states since k_row_states jumps to the row's first draw and takes the noise accumulators from the rand()
window there (csrc/ntsc_rowstate_lookback.hpp; the host sweep: tests/test_rowstate_lookback_host.py): widths 16 (the
narrowest frame the library takes), 24, 40 and 64 -- row strides below, at and above the look-back lengths and the
31-word window for luma (W draws per row) and chroma (2 W, or 2 (W / 2) in the YUV422P tool) --, heights 2 to 20, a
stream that begins at rand() position 0, where the first rows have fewer than 31 draws behind them, and far into it,
small and large noise amplitudes, the default look-back and the test hook's 2 / 2, which sends most rows through the
backward extension.  One launch of 8 fields and 8 launches of one field (either takes k_field_row_setup where the
per-field draws are on, k_row_states where they are off) == the oracle byte for byte (tolerance 0: integer pixels in and
out, the reference's operation order), with rng_pos checked."""
import numpy as np
import pytest

import _libs as L
import ntscsim

pytestmark = pytest.mark.gpu

WIDTHS = (16, 24, 40, 64)
HEIGHTS = (2, 3, 7, 20)
POSITIONS = (0, 5000003)
N = 8

# luma noise 4 / 100, chroma noise 16 / 200; `states_only`: no head switching, phase noise or dropout, so that the setup
# is k_row_states alone and not the merged k_field_row_setup
NOISE = [
    ("n4_c16", ["-vhs", "-noise", "4", "-chroma-noise", "16"], "k_field_row_setup"),
    ("n100_c200", ["-vhs", "-noise", "100", "-chroma-noise", "200"], "k_field_row_setup"),
    ("states_only", ["-vhs", "-noise", "100", "-chroma-noise", "16", "-vhs-head-switching", "0", "-chroma-phase-noise", "0",
                     "-chroma-dropout", "0"], "k_row_states"),
]

_JOBS = [(k // 2, k, (k & 1) ^ 1, k) for k in range(N)]


def _expected_bgra(p, w, h, pos):
    frames = [L.noise_frame(w, h, 0x10B4C + 977 * w + 31 * h + i) for i in range(N // 2)]
    o = L.OracleStream(p)
    o.skip(pos)
    exp = np.zeros((N, h, w, 4), np.uint8)
    for (si, di, field, fieldno) in _JOBS:
        o.field(exp[di], frames[si], field, fieldno)
    return frames, exp, o.rng_pos


def _check_bgra(sim, torch, frames, exp, end_pos, pos, one_launch, setup, what):
    src = torch.from_numpy(np.stack(frames)).cuda()
    dst = torch.zeros(exp.shape, dtype=torch.uint8, device="cuda")
    sim.rng_pos = pos
    if one_launch:
        sim.fields(src, dst, _JOBS)
        assert setup in sim.last_kernels(), (what, sim.last_kernels())
    else:
        for j in _JOBS:
            sim.fields(src, dst, [j])
    sim.sync()
    got = dst.cpu().numpy()
    bad = int((got != exp).sum())
    assert bad == 0, "%s: %d mismatching bytes, first at %s" % (what, bad, tuple(int(i[0]) for i in np.nonzero(got != exp)))
    assert sim.rng_pos == end_pos, what


@pytest.mark.parametrize("name,flags,setup", NOISE, ids=[n[0] for n in NOISE])
def test_bgra_row_states_equal_the_oracle(name, flags, setup):
    import torch
    p = L.make_params(flags)
    sim = ntscsim.FieldSimulator(params=p)
    try:
        for w in WIDTHS:
            for h in HEIGHTS:
                for pos in POSITIONS:
                    frames, exp, end_pos = _expected_bgra(p, w, h, pos)          # one reference for the four runs
                    for hook in (False, True):
                        sim.debug_set_warmup(2, 2) if hook else sim.debug_set_warmup(0, 0)
                        for one_launch in (True, False):
                            what = "%s %dx%d pos %d hook %d one launch %d" % (name, w, h, pos, hook, one_launch)
                            _check_bgra(sim, torch, frames, exp, end_pos, pos, one_launch, setup, what)
    finally:
        sim.close()


def _expected_422(p, w, h, pos):
    """Four frames, both fields of each, processed in place in the tool's order.  Returns the frames before, the frames
    after, every field's stream position and the position behind the last."""
    before = [L.yuv_noise(w, h, 0x422 + 131 * w + 7 * h + i, pad=16) for i in range(N // 2)]
    after = [f.copy() for f in before]
    o = L.TocompOracleStream(p, L.OOB_MEMORY)
    o.skip(pos)
    at = []
    for (si, _, field, fieldno) in _JOBS:
        at.append(o.rng_pos)
        o.process(after[si], field, fieldno)
    return before, after, at, o.rng_pos


def _check_422(sim, torch, before, after, at, end_pos, pos, one_launch, setup, what):
    w, h = before[0].w, before[0].h
    whole, dev = [], []
    for f in before:
        t = torch.from_numpy(f.buf.copy()).cuda()
        whole.append(t)
        dev.append([t[f.off[i]:f.off[i] + f.ls[i] * h].view(h, f.ls[i]) for i in range(3)])
    sim.rng_pos = pos
    if one_launch:
        sim.fields422([{"dst": dev[si], "field": field, "fieldno": fieldno, "rng_pos": at[k]}
                       for k, (si, _, field, fieldno) in enumerate(_JOBS)], w, h)
        assert setup in sim.last_kernels(), (what, sim.last_kernels())
    else:
        for (si, _, field, fieldno) in _JOBS:
            sim.fields422([{"dst": dev[si], "field": field, "fieldno": fieldno}], w, h)
    sim.sync()
    for i, f in enumerate(after):
        got = whole[i].cpu().numpy()
        bad = int((got != f.buf).sum())
        assert bad == 0, "%s frame %d: %d mismatching bytes, first at %d" % (what, i, bad, int(np.argmax(got != f.buf)))
    assert sim.rng_pos == end_pos, what


@pytest.mark.parametrize("name,flags,setup", NOISE, ids=[n[0] for n in NOISE])
def test_yuv422p_row_states_equal_the_oracle(name, flags, setup):
    import torch
    p = L.make_params_tocomp(flags)
    sim = ntscsim.FieldSimulator(params=p)
    try:
        for w in WIDTHS:
            for h in HEIGHTS:
                for pos in POSITIONS:
                    before, after, at, end_pos = _expected_422(p, w, h, pos)
                    for hook in (False, True):
                        sim.debug_set_warmup(2, 2) if hook else sim.debug_set_warmup(0, 0)
                        for one_launch in (True, False):
                            what = "%s 422 %dx%d pos %d hook %d one launch %d" % (name, w, h, pos, hook, one_launch)
                            _check_422(sim, torch, before, after, at, end_pos, pos, one_launch, setup, what)
    finally:
        sim.close()
