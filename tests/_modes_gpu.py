"""What tests/test_float_model_gpu.py and tests/test_fast32_model_gpu.py share: the model over a list of jobs, one
device launch of the same jobs, and the two comparisons (admissible set against real64, equality against fast32).
Test infrastructure only."""
import numpy as np
import pytest

import _modes as M

FILL = 0x77


def q(x):
    """the final truncation and clamp of a channel value in output LSB"""
    return np.clip(np.trunc(x), 0, 255).astype(np.int16)


def model(flavour, p, srcs, jobs, h, w, il, tff, taps=None):
    """the model over the jobs, one rand() stream: (rand() position, per field the flavour's outputs, its frames)"""
    m = M.ModelStream(p, flavour)
    outs, frames = [], []
    for si, field, fieldno in jobs:
        d = np.full((h, w, 4), FILL, np.uint8)
        outs.append(m.field(d, srcs[si], field, fieldno, il, tff, taps=taps) if taps else m.field(d, srcs[si], field, fieldno, il, tff))
        frames.append(d)
    return m.rng_pos, outs, frames


def first(bad):
    return tuple(int(v) for v in np.argwhere(bad)[0])


def check_float_fields(got, comp, outs, jobs, what, delta_out, delta_comp):
    """got: uint8 [n, H, W, 4]; comp: float32 [n, Lslot, W] (or None); outs: real64's outputs per field"""
    for k, (si, field, fieldno) in enumerate(jobs):
        v = outs[k]["v"]                                  # [L, W, 3] r, g, b
        rows = v.shape[0]
        if comp is not None and rows:
            dc = np.abs(comp[k, :rows].astype(np.float64) - outs[k]["composite"])
            if dc.max() > delta_comp:
                r, x = first(dc > delta_comp)
                pytest.fail("%s: composite field %d row %d (frame row %d) x %d: kernel %r model %r" %
                            (what, k, r, field + 2 * r, x, float(comp[k, r, x]), float(outs[k]["composite"][r, x])))
        assert (got[k][1 - field::2] == FILL).all(), (what, k, "other field's rows")
        mine = got[k][field::2]
        assert not mine[..., 3].any(), (what, k, "alpha")
        b = mine[..., 2::-1].astype(np.int16)             # memory order B, G, R -> r, g, b
        lo, hi = q(v - delta_out), q(v + delta_out)
        bad = (b != lo) & (b != hi)
        if bad.any():
            r, x, c = first(bad)
            pytest.fail("%s: output (field, row, x, channel, v, byte) = (%d, %d, %d, %s, %.6f, %d); %d channels off" %
                        (what, k, r, x, "rgb"[c], float(v[r, x, c]), int(b[r, x, c]), int(bad.sum())))


def check_equal_fast32(got, compi, outs, frames, jobs, what):
    """byte for byte against the fast32 flavour, the int32 composite plane against its composite_y tap"""
    for k, (si, field, fieldno) in enumerate(jobs):
        rows = outs[k]["composite_y"].shape[0]
        if compi is not None and rows:
            bad = compi[k, :rows] != outs[k]["composite_y"]
            if bad.any():
                r, x = first(bad)
                pytest.fail("%s: composite field %d row %d x %d: kernel %d model %d (%d samples differ)" %
                            (what, k, r, x, int(compi[k, r, x]), int(outs[k]["composite_y"][r, x]), int(bad.sum())))
        bad = got[k] != frames[k]
        if bad.any():
            y, x, c = first(bad)
            pytest.fail("%s: output field %d frame row %d x %d byte %d: kernel %d model %d (%d bytes differ)" %
                        (what, k, y, x, c, int(got[k][y, x, c]), int(frames[k][y, x, c]), int(bad.sum())))


def is_fp(kern):
    """the names of the all-float kernels among those of a launch"""
    return [k_ for k_ in kern if k_.endswith("_fp") or "_fp<" in k_ or k_ == "k_decode_fp2"]


def launch(sim, srcs, jobs, h, w, il, tff, pad=0):
    """one ntscsim_fields_device() call over the jobs: (frames [n, H, W, 4], kernel names, composite plane [n, Lslot, W]).
    pad: pixels per row of the device buffers (0: rows are W pixels) -- an odd W on 16-byte-aligned rows"""
    import torch
    pw = pad or w
    src = torch.zeros((len(srcs), h, pw, 4), dtype=torch.uint8, device="cuda")
    src[:, :, :w] = torch.from_numpy(np.stack(srcs)).cuda()
    dst = torch.full((len(jobs), h, pw, 4), FILL, dtype=torch.uint8, device="cuda")
    sim.fields(src[:, :, :w], dst[:, :, :w], [(si, k, field, fieldno) for k, (si, field, fieldno) in enumerate(jobs)],
               interlaced=il, tff=tff)
    sim.sync()
    got = dst.cpu().numpy()
    assert (got[:, :, w:] == FILL).all(), "row padding written"
    return np.ascontiguousarray(got[:, :, :w]), sim.last_kernels(), sim.debug_composite(len(jobs), w, h)
