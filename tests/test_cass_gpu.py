"""The device half of the cassette stage (ntscsim_cass_*: k_audio_hiss, k_cass_front, k_cass_front_verify, k_cass_conv,
k_cass_back, k_cass_back_verify) against the host checker on the same host (tests/cass_chain_check.cpp over
csrc/cass_chain.hpp, run serially with every tap of the FIR; tests/test_cass_ref.py pins it to the reference's own lines),
byte for byte and state bit for state bit, the FIR's history included: the chain is exact arithmetic, so the tolerance is
zero.  The rand() position of the ctx is compared as well, and the device's repair counts with the host plan's.

Shapes: no track is longer than 12,000 frames.  The switch sets run with -high 100 where they would have a 20 Hz
high-pass, so that the default front warm-up is 5,056 frames and 12,000 frames give segments beyond it; the pipeline-edge
runs are 1,500 frames with debug_set_plan, so that segments shorter than the 17-lane pipeline is deep, fill and drain
across the warm-up / own boundary and every packing of three segments per wavefront are met in milliseconds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _cass_ref as A
import _libs as L
import ntscsim
from ntscsim import _capi

pytestmark = pytest.mark.gpu

SWITCH_SETS = sorted({tuple(v[0]) for v in A.CASES.values()})
TILE = 256                                                                       # frames of a workgroup of k_cass_conv


@pytest.fixture(scope="module")
def sim():
    s = ntscsim.FieldSimulator(device=0)
    yield s
    s.close()


def params(flags):
    return _capi.make_cass_params(list(flags))


def run_device(chain, audio, blocks=None):
    import torch
    src = torch.from_numpy(np.ascontiguousarray(audio)).cuda()
    dst = torch.full_like(src, 0x5555)
    chain.process(src, dst, blocks)
    chain.sync()
    assert torch.equal(src.cpu(), torch.from_numpy(np.ascontiguousarray(audio))), "the call wrote its source"
    return dst.cpu().numpy()


def bits(v):
    return np.array(v, np.float64).view(np.uint64)


def assert_same(chain, got, want, want_state, what=""):
    bad = int((got != want).sum())
    first = int(np.argmax((got != want).reshape(-1))) if bad else -1
    assert bad == 0, "%s: %d wrong samples, first at %d" % (what, bad, first)
    vals, count, hist = chain.state
    wvals, wcount, whist = want_state
    assert count == wcount, what
    assert (bits(vals) == wvals).all(), "%s: filter states %s" % (what, np.nonzero(bits(vals) != wvals)[0])
    assert (bits(hist).reshape(-1, 2) == whist).all(), "%s: history" % what


def test_the_feature_exists(sim):
    """One 4096-frame call at the default settings equals the checker."""
    cp = params([])
    a = A.make_input("music", 4096, 2, 21)
    want, st, pos = A.run_checker(cp, a)
    sim.rng_pos = 0
    chain = ntscsim.Cassette(cp, sim=sim)
    got = run_device(chain, a)
    assert_same(chain, got, want, st)
    assert sim.rng_pos == pos == 8192


@pytest.mark.parametrize("flags", SWITCH_SETS, ids=lambda f: " ".join(f) or "default")
def test_bytes_state_and_rand_position(sim, flags):
    cp = params(flags)
    if cp.highpass_hz < 100:
        cp = params(list(flags) + ["-high", "100"])
    frames = 12000
    a = A.make_input("loud" if cp.preemphasis else "music", frames, 2, 31 + len(flags))
    want, st, pos = A.run_checker(cp, a, rng_pos=1000)
    sim.rng_pos = 1000
    chain = ntscsim.Cassette(cp, sim=sim)
    wf, wb = chain.default_warmups()
    assert wf <= 5056 and wb == 64
    got = run_device(chain, a)
    assert_same(chain, got, want, st, str(flags))
    assert sim.rng_pos == pos
    stats = chain.stats()
    print("segments %d repaired %d / %d" % stats)
    assert stats[0] == 3 and stats[0] * 4096 > wf + 4096                        # the last segment starts from zeros, a full warm-up early
    assert stats == A.plan_stats(cp, a, 4096, wf, wb, rng_pos=1000)
    assert stats[1] == 0 and stats[2] == 0                                      # tests/test_cass_chain_host.py: both passes converge in time


@pytest.mark.parametrize("which", ["default_deemph", "bad_deck_mono_both"])
def test_stage_pipeline_edges(sim, which):
    cp = params({"default_deemph": ["-deemphasis", "1"], "bad_deck_mono_both": ["-preset", "3", "-mono", "-preemphasis", "1", "-deemphasis", "1"]}[which])
    a = A.make_input("music", 1500, 2, 5)
    want, st, pos = A.run_checker(cp, a, rng_pos=3)
    chain = ntscsim.Cassette(cp, sim=sim)
    for seg in (1, 2, 63, 64, 65):
        for wf, wb in ((0, 0), (1, 64), (15, 2), (16, 1), (17, 17), (64, 3)):
            chain.set_plan(seg, wf, wb)
            chain.reset()
            sim.rng_pos = 3
            got = run_device(chain, a)
            assert_same(chain, got, want, st, "L %d W %d %d" % (seg, wf, wb))
            assert sim.rng_pos == pos
            stats = chain.stats()
            assert stats[0] == (1500 + seg - 1) // seg
            if (wf, wb) == (0, 0) or seg == 64:
                assert stats == A.plan_stats(cp, a, seg, wf, wb, rng_pos=3), "L %d W %d %d" % (seg, wf, wb)
            if (wf, wb) == (0, 0):                                              # every segment but the first is repaired, the bytes are the same
                assert stats[1] == stats[0] - 1 and stats[2] >= stats[0] - 1 - cp.taps
    # 1, 2, 3, 4 and 7 segments in wavefronts of three, the last of one frame
    for frames in (64, 128, 192, 193, 6 * 64 + 1):
        w2, s2, _ = A.run_checker(cp, a[:frames], rng_pos=3)
        chain.set_plan(64, 20, 20)
        chain.reset()
        sim.rng_pos = 3
        got = run_device(chain, a[:frames])
        assert_same(chain, got, w2, s2, "%d frames" % frames)
        assert chain.stats()[0] == (frames + 63) // 64


@pytest.mark.parametrize("flags", [(), ("-deemphasis", "1"), ("-preset", "3"), ("-preset", "3", "-deemphasis", "1", "-mono")], ids=lambda f: " ".join(f) or "default")
def test_lengths_at_the_tile_and_at_the_taps(sim, flags):
    cp = params(flags)
    chain = ntscsim.Cassette(cp, sim=sim)
    a = A.make_input("music", 2 * TILE + 1, 2, 7)
    t = cp.taps
    for frames in (1, t - 2, t - 1, t, t + 1, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1):
        want, st, pos = A.run_checker(cp, a[:frames], rng_pos=11)
        chain.reset()
        sim.rng_pos = 11
        got = run_device(chain, a[:frames])
        assert_same(chain, got, want, st, "%d frames" % frames)
        assert sim.rng_pos == pos
    # then as consecutive calls of those lengths: the history is carried, partly from the call before the last
    cuts = [1, t - 2, t - 1, t, TILE - 1, 1, TILE + 1]
    total = sum(cuts)
    a = A.make_input("music", total, 2, 8)
    want, st, pos = A.run_checker(cp, a, rng_pos=11)
    chain.reset()
    sim.rng_pos = 11
    got, at = [], 0
    for n in cuts:
        got.append(run_device(chain, a[at:at + n]))
        at += n
    assert_same(chain, np.concatenate(got), want, st, "calls of %s" % cuts)
    assert sim.rng_pos == pos


@pytest.mark.parametrize("block", [1, 3, 5])
def test_small_calls_carry_the_halo_with_57_taps(sim, block):
    cp = params(["-preset", "3", "-deemphasis", "1"])
    assert cp.taps == 57
    frames = 40 * block + 2
    a = A.make_input("music", frames, 2, 9 + block)
    want, st, pos = A.run_checker(cp, a, rng_pos=5, block=block)
    one, _, _ = A.run_checker(cp, a, rng_pos=5)
    assert (want == one).all()
    chain = ntscsim.Cassette(cp, sim=sim)
    sim.rng_pos = 5
    got = [run_device(chain, a[at:at + block]) for at in range(0, frames, block)]   # the halo of a call spans the 11 .. 56 calls before it
    assert_same(chain, np.concatenate(got), want, st, "calls of %d" % block)
    assert sim.rng_pos == pos
    # and as descriptors of one call
    chain.reset()
    sim.rng_pos = 5
    got = run_device(chain, a, [(min(block, frames - at), None) for at in range(0, frames, block)])
    assert_same(chain, got, want, st, "descriptors of %d" % block)


def test_repair_path(sim):
    cp = params(["-deemphasis", "1"])
    a = A.make_input("music", 3000, 2, 6)
    want, st, _ = A.run_checker(cp, a)
    chain = ntscsim.Cassette(cp, sim=sim)
    chain.set_plan(256, 0, 0)
    sim.rng_pos = 0
    got = run_device(chain, a)
    assert_same(chain, got, want, st)
    assert chain.stats() == (12, 11, 11)
    # silence without hiss: a zero state IS the true state, nothing to repair
    cp0 = params(["-audio-hiss", "-200", "-deemphasis", "1"])
    assert cp0.hiss_level == 0
    z = np.zeros((3000, 2), np.int16)
    chain0 = ntscsim.Cassette(cp0, sim=sim)
    chain0.set_plan(256, 0, 0)
    got = run_device(chain0, z)
    assert not got.any()
    assert chain0.stats() == (12, 0, 0)


def test_blocks_calls_and_resume(sim):
    cp = params(["-preset", "0", "-preemphasis", "1", "-deemphasis", "1"])       # 25 taps, 100 Hz
    a = A.make_input("music", 9000, 2, 8)
    blocks = [(1500, 700), (0, 5), (1, 100000), (2999, None), (1700, 12), (800, 12), (2000, 1 << 33)]   # positions go backwards
    spec = "blocks=" + ",".join("%d:%s" % (n, "a" if p is None else p) for n, p in blocks)
    want, st, pos = A.run_checker(cp, a, block=spec)
    chain = ntscsim.Cassette(cp, sim=sim)
    chain.set_plan(1000, 200, 30)                                               # warm-ups cross block boundaries
    sim.rng_pos = 1
    got = run_device(chain, a, blocks)
    assert_same(chain, got, want, st, "7 blocks")
    assert sim.rng_pos == pos == (1 << 33) + 4000
    # at the default plan too
    chain.set_plan(0, 0, 0)
    chain.reset()
    got = run_device(chain, a, blocks)
    assert_same(chain, got, want, st, "7 blocks, default plan")
    # two calls are one call
    one, st1, pos1 = A.run_checker(cp, a, rng_pos=50)
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
    chain2 = ntscsim.Cassette(cp, sim=sim)
    assert chain2.state == (tuple([0.0] * 28), 0, tuple([(0.0, 0.0)] * 24))
    chain2.state = saved
    sim.rng_pos = at
    got = np.concatenate([first, run_device(chain2, a[4001:])])
    assert_same(chain2, got, one, st1, "resumed")


def test_start_at_a_count_of_hours(sim):
    cp = params(["-preset", "3"])
    a = A.make_input("music", 3000, 2, 9)
    want, st, _ = A.run_checker(cp, a, count0=3000000000)
    zero, _, _ = A.run_checker(cp, a, count0=0)
    assert int((want != zero).sum()) > 100                                      # the head tilt's phase is audible
    chain = ntscsim.Cassette(cp, sim=sim)
    chain.state = (tuple([0.0] * 28), 3000000000, ())
    sim.rng_pos = 0
    got = run_device(chain, a)
    assert_same(chain, got, want, st)


def test_host_call_in_place(sim):
    cp = params(["-preset", "4", "-deemphasis", "1"])
    a = A.make_input("music", 2500, 2, 10)
    want, st, pos = A.run_checker(cp, a, rng_pos=9)
    chain = ntscsim.Cassette(cp, sim=sim)
    sim.rng_pos = 9
    raw = np.zeros(2 * a.size + 3, np.uint8)
    view = raw[1:1 + 2 * a.size].view(np.int16).reshape(a.shape)                # an odd address; source and destination are the same
    assert view.ctypes.data % 2 == 1
    view[:] = a
    chain.host(view)
    assert_same(chain, np.array(view), want, st)
    assert raw[0] == 0 and not raw[1 + 2 * a.size:].any()
    assert sim.rng_pos == pos


def test_error_codes(sim):
    import torch
    lib = sim._lib
    cp = params([])
    fresh = ntscsim.FieldSimulator(device=0)
    try:
        d = (_capi.CassDesc * 1)()
        st = _capi.CassState()
        assert lib.ntscsim_cass_device(fresh._h, d, 1, None) == _capi.E_ARG    # no bind
        assert lib.ntscsim_cass_host(fresh._h, None, 0) == _capi.E_ARG
        assert lib.ntscsim_cass_reset(fresh._h) == _capi.E_ARG
        assert lib.ntscsim_cass_get_state(fresh._h, C.byref(st)) == _capi.E_ARG
        assert lib.ntscsim_cass_debug_set_plan(fresh._h, 1, 1, 1) == _capi.E_ARG
    finally:
        fresh.close()
    chain = ntscsim.Cassette(cp, sim=sim)
    buf = torch.zeros(4096, dtype=torch.int16, device="cuda")
    base = buf.data_ptr()
    sim.rng_pos = 5

    def call(src, dst, samples, n=1):
        d = (_capi.CassDesc * 2)()
        d[0].src, d[0].dst, d[0].samples, d[0].rng_pos = src, dst, samples, _capi.RNG_AUTO
        d[1].src, d[1].dst, d[1].samples, d[1].rng_pos = base + 4096, base + 6000, 100, _capi.RNG_AUTO
        return lib.ntscsim_cass_device(sim._h, d, n, None)

    assert call(base, base, 100) == _capi.E_ARG                                 # in place
    assert call(base, base + 396, 100) == _capi.E_ARG                           # dst overlaps the end of src
    assert call(base, base + 4096 + 396, 100, 2) == _capi.E_ARG                 # dst overlaps the src of another block
    assert call(None, base, 100) == _capi.E_ARG
    assert call(base, None, 100) == _capi.E_ARG
    assert call(base + 1, base + 2000, 100) == _capi.E_ARG                      # odd pointers
    assert call(base, base + 2001, 100) == _capi.E_ARG
    assert lib.ntscsim_cass_device(sim._h, None, 1, None) == _capi.E_ARG
    assert sim.rng_pos == 5                                                     # a refused call draws nothing
    assert call(None, None, 0) == _capi.OK                                      # an empty block needs no pointers
    assert call(base, base + 400, 100) == _capi.OK
    sim.sync()
    assert sim.rng_pos == 205
    assert lib.ntscsim_cass_get_state(sim._h, None) == lib.ntscsim_cass_set_state(sim._h, None) == _capi.E_ARG
    st = _capi.CassState()
    assert lib.ntscsim_cass_get_state(sim._h, C.byref(st)) == _capi.OK and st.taps == 8 and st.count == 100
    st.taps = 9
    assert lib.ntscsim_cass_set_state(sim._h, C.byref(st)) == _capi.E_ARG       # a state of other params
    assert lib.ntscsim_cass_debug_kernel_ms(sim._h, (C.c_float * 8)()) == _capi.E_ARG   # nothing was timed
    for field, value in (("channels", 1), ("passes", 5), ("rate", 0), ("lowpass_hz", 0.0), ("highpass_hz", -1.0), ("taps", 9), ("taps", 0), ("hiss_level", -1)):
        bad = _capi.CassParams.from_buffer_copy(cp)
        setattr(bad, field, value)
        assert lib.ntscsim_cass_bind(sim._h, C.byref(bad)) == _capi.E_PARAM, field
    bad = _capi.CassParams.from_buffer_copy(cp)
    bad.struct_size = 8
    assert lib.ntscsim_cass_bind(sim._h, C.byref(bad)) == _capi.E_ARG
    assert lib.ntscsim_cass_bind(sim._h, None) == _capi.E_ARG


def test_kernel_times(sim):
    cp = params(["-preset", "3", "-deemphasis", "1"])
    chain = ntscsim.Cassette(cp, sim=sim)
    chain.debug_time_kernels(True)
    a = A.make_input("music", 6000, 2, 3)
    run_device(chain, a)
    ms = chain.kernel_ms()
    print(ms)
    assert len(ms) == 8 and all(v >= 0 for v in ms) and ms[3] > 0 and ms[5] > 0 and ms[6] > 0
    assert sim.last_kernels() == ["k_audio_hiss", "k_cass_front", "k_cass_front_verify", "k_cass_conv", "k_cass_back", "k_cass_back_verify"]
    chain.debug_time_kernels(False)
    chain2 = ntscsim.Cassette(params(["-audio-hiss", "-200"]), sim=sim)
    run_device(chain2, a)
    assert sim.last_kernels() == ["k_cass_front", "k_cass_front_verify", "k_cass_conv"]


def test_audio_and_cassette_on_one_ctx(sim):
    """Both stages bound on one ctx: they share the rand() position and nothing else."""
    import _audio_ref as AU
    ap, _ = _capi.make_audio_params([])
    cp = params(["-preset", "0", "-deemphasis", "1"])
    a = A.make_input("music", 3000, 2, 12)
    audio = ntscsim.AudioChain(ap, sim=sim)
    cass = ntscsim.Cassette(cp, sim=sim)
    sim.rng_pos = 40
    want_a1, st_a1, pos1 = AU.run_checker(ap, a[:1500], rng_pos=40)
    got_a1 = run_device(audio, a[:1500])
    want_c, st_c, pos2 = A.run_checker(cp, a, rng_pos=pos1)
    got_c = run_device(cass, a)
    # the audio stage goes on where it stood, as if the cassette call had not been
    want_a, st_a, _ = AU.run_checker(ap, a, rng_pos=40, block="blocks=1500:40,1500:%d" % pos2)
    got_a2 = run_device(audio, a[1500:])
    assert sim.rng_pos == pos2 + 3000
    assert (got_a1 == want_a1).all() and (np.concatenate([got_a1, got_a2]) == want_a).all()
    vals, count = audio.state
    assert count == st_a[1] and (AU.state_bits(vals) == AU.state_bits(st_a[0])).all()
    assert_same(cass, got_c, want_c, st_c)
    # a fresh bind of one resets that one alone
    ntscsim.AudioChain(ap, sim=sim)
    assert_same(cass, got_c, want_c, st_c)


def test_cli_on_the_gpu_equals_its_host_fallback(tmp_path):
    exe = os.path.join(L.PKG, "cassette_cli")
    a = A.make_input("music", 5000, 2, 12)
    inp = tmp_path / "in.s16"
    a.tofile(str(inp))
    outs = []
    for extra in (["--host"], [], ["--block", "1601"]):
        out = tmp_path / ("out%d.s16" % len(outs))
        r = subprocess.run([exe] + extra + ["--rng-pos", "77", "-preset", "3", "-mono", "-deemphasis", "1", "-i", str(inp), "-o", str(out)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert ("on the host" if extra == ["--host"] else "on the device") in r.stderr, r.stderr
        assert "rand() position 10077" in r.stderr
        outs.append(np.fromfile(str(out), np.int16))
    assert outs[0].size == 10000 and (outs[0] == outs[1]).all() and (outs[0] == outs[2]).all()
