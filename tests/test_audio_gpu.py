"""The device half of the audio stage (ntscsim_audio_*: k_audio_hiss, k_audio_pulses, k_audio_segments,
k_audio_verify_repair) against the host checker (tests/audio_chain_check.cpp over csrc/audio_chain.hpp, which
tests/test_audio_ref.py pins to the reference's own lines), byte for byte and state bit for state bit: the chain is
exact arithmetic, so the tolerance is zero.  The rand() position of the ctx is compared as well.

Shapes: 60,000 frames (20 Hz presets) and 12,000 (100 Hz presets) are the smallest that give more than one segment
beyond the default warm-up (25,280 / 5,056 frames, segments of 4,096); the pipeline-edge runs are 3,000 frames with
debug_set_plan, so that segments shorter than the 21-lane pipeline is deep, fill and drain across the warm-up / own
boundary and every packing of three segments per wavefront are met in milliseconds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _audio_ref as A
import _libs as L
import ntscsim
from ntscsim import _capi

pytestmark = pytest.mark.gpu

SWITCH_SETS = sorted({tuple(v[0]) for v in A.CASES.values()})


@pytest.fixture(scope="module")
def sim():
    s = ntscsim.FieldSimulator(device=0)
    yield s
    s.close()


def params(flags, **edit):
    ap, _ = _capi.make_audio_params(list(flags))
    for k, v in edit.items():
        setattr(ap, k, v)
    return ap


def run_device(chain, audio, blocks=None):
    import torch
    src = torch.from_numpy(np.ascontiguousarray(audio)).cuda()
    dst = torch.full_like(src, 0x5555)
    chain.process(src, dst, blocks)
    chain.sync()
    assert torch.equal(src.cpu(), torch.from_numpy(np.ascontiguousarray(audio))), "the call wrote its source"
    return dst.cpu().numpy()


def assert_same(chain, got, want, want_state, what=""):
    bad = int((got != want).sum())
    first = int(np.argmax((got != want).reshape(-1))) if bad else -1
    assert bad == 0, "%s: %d wrong samples, first at %d" % (what, bad, first)
    vals, count = chain.state
    assert count == want_state[1], what
    assert (A.state_bits(vals) == A.state_bits(want_state[0])).all(), what


def stereo_linear():
    """linear audio with two channels: nothing in the tools sets it, the chain handles it (buzz, per-channel boost)"""
    return params(["-vhs", "-vhs-hifi", "0"], channels=2)


def test_the_feature_exists(sim):
    """One 4096-frame stereo call at the default preset equals the checker."""
    ap = params([])
    a = A.make_input("music", 4096, 2, 21)
    want, st, pos = A.run_checker(ap, a)
    sim.rng_pos = 0
    chain = ntscsim.AudioChain(ap, sim=sim)
    got = run_device(chain, a)
    assert_same(chain, got, want, st)
    assert sim.rng_pos == pos == 8192


@pytest.mark.parametrize("flags", SWITCH_SETS, ids=lambda f: " ".join(f) or "default")
def test_bytes_state_and_rand_position(sim, flags):
    ap = params(flags)
    frames = 60000 if ap.highpass_hz == 20 else 12000
    a = A.make_input("loud" if "-vhs" in flags else "music", frames, ap.channels, 31 + len(flags))
    want, st, pos = A.run_checker(ap, a, rng_pos=1000)
    sim.rng_pos = 1000
    chain = ntscsim.AudioChain(ap, sim=sim)
    got = run_device(chain, a)
    assert_same(chain, got, want, st, str(flags))
    assert sim.rng_pos == pos
    segments, repaired = chain.stats()
    print("segments %d repaired %d" % (segments, repaired))
    if ap.enabled:
        assert segments == (frames + 4095) // 4096 and segments * 4096 > chain.default_warmup() + 4096
        assert repaired == 0                                                    # tests/test_audio_chain_host.py: the chain converges in time


@pytest.mark.parametrize("which", ["mono", "stereo", "stereo_linear"])
def test_stage_pipeline_edges(sim, which):
    ap = {"mono": lambda: params(["-vhs-hifi", "0", "-vhs-speed", "lp"]), "stereo": lambda: params([]), "stereo_linear": stereo_linear}[which]()
    a = A.make_input("music", 3000, ap.channels, 5)
    want, st, pos = A.run_checker(ap, a, count0=0, rng_pos=3)
    chain = ntscsim.AudioChain(ap, sim=sim)
    for seg in (1, 2, 63, 64, 65):
        for warm in (0, 1, 19, 20, 21, 64):
            chain.set_plan(seg, warm)
            chain.reset()
            sim.rng_pos = 3
            got = run_device(chain, a)
            assert_same(chain, got, want, st, "L %d W %d" % (seg, warm))
            assert sim.rng_pos == pos
            assert chain.stats()[0] == (3000 + seg - 1) // seg
            assert chain.stats() == A.plan_stats(ap, a, seg, warm, rng_pos=3), "L %d W %d" % (seg, warm)
    # 1, 2, 3, 4 and 7 segments in wavefronts of three, the last of one frame
    for frames in (64, 128, 192, 193, 6 * 64 + 1):
        w2, s2, _ = A.run_checker(ap, a[:frames], rng_pos=3)
        chain.set_plan(64, 20)
        chain.reset()
        sim.rng_pos = 3
        got = run_device(chain, a[:frames])
        assert_same(chain, got, w2, s2, "%d frames" % frames)
        assert chain.stats()[0] == (frames + 63) // 64
        assert chain.stats() == A.plan_stats(ap, a[:frames], 64, 20, rng_pos=3), "%d frames" % frames


def test_repair_path(sim):
    ap = params([])
    a = A.make_input("music", 3000, 2, 6)
    want, st, _ = A.run_checker(ap, a)
    chain = ntscsim.AudioChain(ap, sim=sim)
    chain.set_plan(256, 0)
    sim.rng_pos = 0
    got = run_device(chain, a)
    assert_same(chain, got, want, st)
    segments, repaired = chain.stats()
    assert segments == 12 and repaired == segments - 1
    assert (segments, repaired) == A.plan_stats(ap, a, 256, 0)
    # silence without hiss: a zero state IS the true state, nothing to repair
    ap0 = params(["-audio-hiss", "-200"])
    assert ap0.hiss_level == 0
    z = np.zeros((3000, 2), np.int16)
    chain0 = ntscsim.AudioChain(ap0, sim=sim)
    chain0.set_plan(256, 0)
    got = run_device(chain0, z)
    assert not got.any()
    assert chain0.stats() == (12, 0) == A.plan_stats(ap0, z, 256, 0)


def test_blocks_calls_and_resume(sim):
    ap = params(["-vhs", "-vhs-hifi", "0"])                                      # mono, buzz, boost, hiss 39
    a = A.make_input("music", 9000, 1, 8)
    blocks = [(1500, 700), (0, 5), (1, 100000), (2999, None), (1700, 12), (800, 12), (2000, 1 << 33)]
    spec = "blocks=" + ",".join("%d:%s" % (n, "a" if p is None else p) for n, p in blocks)
    want, st, pos = A.run_checker(ap, a, block=spec)
    chain = ntscsim.AudioChain(ap, sim=sim)
    chain.set_plan(1000, 200)                                                   # warm-ups cross block boundaries
    sim.rng_pos = 1
    got = run_device(chain, a, blocks)
    assert_same(chain, got, want, st, "7 blocks")
    assert sim.rng_pos == pos == (1 << 33) + 2000
    # at the default plan too
    chain.set_plan(0, 0)
    chain.reset()
    got = run_device(chain, a, blocks)
    assert_same(chain, got, want, st, "7 blocks, default plan")
    # two calls are one call
    one, st1, pos1 = A.run_checker(ap, a, rng_pos=50)
    chain.reset()
    sim.rng_pos = 50
    got = np.concatenate([run_device(chain, a[:4001]), run_device(chain, a[4001:])])
    assert_same(chain, got, one, st1, "two calls")
    assert sim.rng_pos == pos1
    # a fresh bind resumes from a saved state
    chain.reset()
    sim.rng_pos = 50
    first = run_device(chain, a[:4001])
    saved, at = chain.state, sim.rng_pos
    chain2 = ntscsim.AudioChain(ap, sim=sim)
    assert chain2.state == (tuple([0.0] * 30), 0)
    chain2.state = saved
    sim.rng_pos = at
    got = np.concatenate([first, run_device(chain2, a[4001:])])
    assert_same(chain2, got, one, st1, "resumed")


@pytest.mark.parametrize("std", ["ntsc", "pal"])
def test_pulse_counts(sim, std):
    ap = params((["-tvstd", "pal"] if std == "pal" else []) + ["-vhs", "-vhs-hifi", "0"])
    chain = ntscsim.AudioChain(ap, sim=sim)
    for count0 in (0, (1 << 31) - 10000, 3000000000):
        got = chain.pulses(count0, 20000)
        want = A.host_pulses(ap, count0, 20000)
        assert (got == want).all(), "count0 %d: %d differ" % (count0, int((got != want).sum()))
        assert 0 < int(want.max()) <= 16


def test_start_at_a_count_of_hours(sim):
    ap = stereo_linear()
    a = A.make_input("quiet", 3000, 2, 9)
    want, st, _ = A.run_checker(ap, a, count0=3000000000)
    chain = ntscsim.AudioChain(ap, sim=sim)
    chain.state = (tuple([0.0] * 30), 3000000000)
    sim.rng_pos = 0
    got = run_device(chain, a)
    assert_same(chain, got, want, st)


def test_fields_and_audio_share_the_stream(sim):
    """Fields, an audio block, fields -- on one ctx, every position NTSCSIM_RNG_AUTO -- against the oracle loop with the
    chain's draws taken out of the same stream at the same place."""
    import torch
    w, h = 96, 32
    p = L.make_params(["-vhs"])
    fs = ntscsim.FieldSimulator(params=p, device=0)
    try:
        ap = params(["-vhs"])
        chain = ntscsim.AudioChain(ap, sim=fs)
        frames = [L.noise_frame(w, h, 77 + i) for i in range(2)]
        jobs = [(k // 2, k, (k & 1) ^ 1, k) for k in range(4)]
        exp = np.zeros((4, h, w, 4), np.uint8)
        o = L.OracleStream(p)
        a = A.make_input("music", 1601, 2, 4)
        src = torch.from_numpy(np.stack(frames)).cuda()
        dst = torch.zeros((4, h, w, 4), dtype=torch.uint8, device="cuda")
        for (si, di, field, fieldno) in jobs[:2]:
            o.field(exp[di], frames[si], field, fieldno)
        fs.fields(src, dst, jobs[:2])
        assert fs.rng_pos == o.rng_pos
        want, st, pos = A.run_checker(ap, a, rng_pos=o.rng_pos)
        o.skip(pos - o.rng_pos)
        got = run_device(chain, a)
        assert fs.rng_pos == o.rng_pos == pos
        for (si, di, field, fieldno) in jobs[2:]:
            o.field(exp[di], frames[si], field, fieldno)
        fs.fields(src, dst, jobs[2:])
        fs.sync()
        assert fs.rng_pos == o.rng_pos
        assert_same(chain, got, want, st)
        assert (dst.cpu().numpy() == exp).all()
    finally:
        fs.close()


def test_host_call_in_place(sim):
    ap = params([])
    a = A.make_input("music", 2500, 2, 10)
    want, st, pos = A.run_checker(ap, a, rng_pos=9)
    chain = ntscsim.AudioChain(ap, sim=sim)
    sim.rng_pos = 9
    raw = np.zeros(2 * a.size + 3, np.uint8)
    view = raw[1:1 + 2 * a.size].view(np.int16).reshape(a.shape)                # an odd address
    assert view.ctypes.data % 2 == 1
    view[:] = a
    chain.host(view)
    assert_same(chain, np.array(view), want, st)
    assert raw[0] == 0 and not raw[1 + 2 * a.size:].any()
    assert sim.rng_pos == pos


def test_error_codes(sim):
    import torch
    lib = sim._lib
    ap = params([])
    fresh = ntscsim.FieldSimulator(device=0)
    try:
        d = (_capi.AudioDesc * 1)()
        assert lib.ntscsim_audio_device(fresh._h, d, 1, None) == _capi.E_ARG   # no bind
        assert lib.ntscsim_audio_host(fresh._h, None, 0) == _capi.E_ARG
    finally:
        fresh.close()
    chain = ntscsim.AudioChain(ap, sim=sim)
    buf = torch.zeros(4096, dtype=torch.int16, device="cuda")
    base = buf.data_ptr()
    sim.rng_pos = 5

    def call(src, dst, samples, n=1):
        d = (_capi.AudioDesc * 2)()
        d[0].src, d[0].dst, d[0].samples, d[0].rng_pos = src, dst, samples, _capi.RNG_AUTO
        d[1].src, d[1].dst, d[1].samples, d[1].rng_pos = base + 4096, base + 6000, 100, _capi.RNG_AUTO
        return lib.ntscsim_audio_device(sim._h, d, n, None)

    assert call(base, base, 100) == _capi.E_ARG                                 # in place
    assert call(base, base + 396, 100) == _capi.E_ARG                           # dst overlaps the end of src
    assert call(base, base + 4096 + 396, 100, 2) == _capi.E_ARG                 # dst overlaps the src of another block
    assert call(None, base, 100) == _capi.E_ARG
    assert call(base, None, 100) == _capi.E_ARG
    assert call(base + 1, base + 2000, 100) == _capi.E_ARG                      # odd pointers
    assert call(base, base + 2001, 100) == _capi.E_ARG
    assert lib.ntscsim_audio_device(sim._h, None, 1, None) == _capi.E_ARG
    assert sim.rng_pos == 5                                                     # a refused call draws nothing
    assert call(None, None, 0) == _capi.OK                                      # an empty block needs no pointers
    assert call(base, base + 400, 100) == _capi.OK
    sim.sync()
    assert sim.rng_pos == 205
    bad = _capi.AudioParams.from_buffer_copy(ap)
    bad.channels = 3
    assert lib.ntscsim_audio_bind(sim._h, C.byref(bad)) == _capi.E_PARAM
    bad.channels, bad.struct_size = 2, 8
    assert lib.ntscsim_audio_bind(sim._h, C.byref(bad)) == _capi.E_ARG


def test_cli_on_the_gpu_equals_its_host_fallback(tmp_path):
    exe = os.path.join(L.PKG, "vhsaudio_cli")
    a = A.make_input("music", 5000, 1, 12)
    inp = tmp_path / "in.s16"
    a.tofile(str(inp))
    outs = []
    for extra in (["--host"], [], ["--block", "1601"]):
        out = tmp_path / ("out%d.s16" % len(outs))
        r = subprocess.run([exe] + extra + ["--rng-pos", "77", "-vhs", "-vhs-hifi", "0", "-i", str(inp), "-o", str(out)], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert ("on the host" if extra == ["--host"] else "on the device") in r.stderr, r.stderr
        assert "rand() position 5077" in r.stderr
        outs.append(np.fromfile(str(out), np.int16))
    assert outs[0].size == 5000 and (outs[0] == outs[1]).all() and (outs[0] == outs[2]).all()
