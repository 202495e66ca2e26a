"""The smallest shapes past each launch threshold of the audio stages (csrc/ntsc_audio.hip, csrc/ntsc_cass.hip,
csrc/audio_hiss.hpp), against the serial host chain (A.run_checker / CR.run_checker, A.run_tracks_checker per track) --
never the code under test -- byte for byte, state bit for state bit (the FIR history included), with the rand() position
and, where stated, the repair counts of the host plan.  The chain is exact arithmetic: the tolerance is zero.

  more than 1024 blocks        k_audio_hiss walks blocks with a stride of gridDim.y = 1024
  more than 1024 tracks        k_audio_track_pulses walks tracks with a stride of gridDim.y = 1024
  the step / jump boundary     audio_hiss_window steps its generator up to 65536 draws and jumps beyond
  2^18 frames                  cass_upload_tilt splits the sin() fill over four threads from there
  65535 * 256 + 300 frames     k_audio_pulses walks frames with a stride of 65535 workgroups of 256
  mixed repairs                "repair segment j, then accept segment j + 1 against the truth the repair produced"

The layouts and the mixed plans are tests/_audio_limits.py's; tests/test_audio_limits_host.py shows on the CPU that they
cross what they are meant to cross and that the plans meet A.mixed_repairs on the host plan."""
import numpy as np
import pytest

import _audio_limits as M
import _audio_ref as A
import _audio_tracks as T
import _cass_ref as CR
import ntscsim
import test_audio_gpu as TA
import test_audio_tracks_gpu as TT
import test_cass_gpu as TC
from ntscsim import _capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    s = ntscsim.FieldSimulator(device=0)
    yield s
    s.close()


@pytest.fixture
def sim(ctx):
    """the module's ctx; a plan that a test set (debug_set_plan outlives a bind) is gone behind it, pass or fail"""
    yield ctx
    if ctx._lib.ntscsim_audio_debug_set_plan(ctx._h, 0, 0) not in (_capi.OK, _capi.E_ARG):      # E_ARG: no audio stage bound yet
        raise AssertionError("ntscsim_audio_debug_set_plan")
    if ctx._lib.ntscsim_cass_debug_set_plan(ctx._h, 0, 0, 0) not in (_capi.OK, _capi.E_ARG):
        raise AssertionError("ntscsim_cass_debug_set_plan")


# ---------------------------------------------------------------------------------------------- B1
@pytest.mark.parametrize("preset", ["mono_lp", "stereo_hifi"])
def test_1500_blocks_through_the_audio_chain(sim, preset):
    ap = T.PRESETS[preset]()
    assert ap.hiss_level != 0
    blocks = M.many_blocks()
    a = A.make_input("music", sum(n for n, _ in blocks), ap.channels, 71)
    want, st, pos = A.run_checker(ap, a, rng_pos=7, block="blocks=" + A.block_spec(blocks))
    chain = ntscsim.AudioChain(ap, sim=sim)
    for plan in ((64, 20), (0, 0)):
        chain.set_plan(*plan)
        chain.reset()
        sim.rng_pos = 7
        got = TA.run_device(chain, a, blocks)
        TA.assert_same(chain, got, want, st, "%d blocks, plan %s" % (len(blocks), plan))
        assert sim.rng_pos == pos
        assert chain.stats()[0] == (len(a) + (plan[0] or 4096) - 1) // (plan[0] or 4096)


def test_1500_blocks_through_the_cassette(sim):
    cp = _capi.make_cass_params(["-preset", "3", "-deemphasis", "1"])
    assert cp.hiss_level != 0 and cp.taps == 57
    blocks = M.many_blocks()
    a = A.make_input("music", sum(n for n, _ in blocks), 2, 72)
    want, st, pos = CR.run_checker(cp, a, rng_pos=7, block="blocks=" + A.block_spec(blocks))
    chain = ntscsim.Cassette(cp, sim=sim)
    for plan in ((64, 20, 20), (0, 0, 0)):
        chain.set_plan(*plan)
        chain.reset()
        sim.rng_pos = 7
        got = TC.run_device(chain, a, blocks)
        TC.assert_same(chain, got, want, st, "%d blocks, plan %s" % (len(blocks), plan))
        assert sim.rng_pos == pos


def test_1500_blocks_in_40_tracks(sim):
    ap = T.PRESETS["mono_lp"]()
    assert ap.hiss_level != 0
    parts = M.spread(M.many_blocks(), 40)
    frames = [sum(n for n, _ in p) for p in parts]
    tracks = T.cut(T.make_tracks(frames, 1, seed=73), frames)
    counts = [100003 * t for t in range(40)]
    want, pos = A.run_tracks_checker(ap, tracks, counts=counts, pos=7, blocks=parts)
    chain = ntscsim.AudioChain(ap, sim=sim)
    chain.set_plan(64, 20)
    states = chain.zero_states(40)
    for t in range(40):
        chain.set_track_state(states, t, (tuple([0.0] * 30), counts[t]))
    sim.rng_pos = 7
    got = TT.run_tracks(chain, tracks, states, parts)
    TT.assert_tracks(got, want, states, what="1500 blocks in 40 tracks")
    assert sim.rng_pos == pos
    assert [s[0] for s in chain.track_stats(40)] == [(f + 63) // 64 for f in frames]


# ---------------------------------------------------------------------------------------------- B2
def test_1100_tracks_with_the_buzz_on(sim):
    """Every track has a state of its own and a sample count 100003 frames from its neighbours', so that the pulse
    counts of track t and of track t + 1024 (one lane's two tracks, were the stride missing) differ."""
    import torch
    ap = T.PRESETS["stereo_linear"]()
    assert ap.buzz != 0 and ap.channels == 2
    n = 1100
    frames = [3 + (t * 11) % 38 for t in range(n)]
    assert min(frames) == 3 and max(frames) == 40
    counts = [100003 * t for t in range(n)]
    assert (A.host_pulses(ap, counts[5], 40) != A.host_pulses(ap, counts[5 + 1024], 40)).any()
    tracks = T.cut(T.make_tracks(frames, 2, seed=74), frames)
    want, pos = A.run_tracks_checker(ap, tracks, counts=counts, pos=7)
    chain = ntscsim.AudioChain(ap, sim=sim)
    chain.set_plan(16, 4)
    raw = np.zeros((n, 31), np.uint64)
    raw[:, 30] = counts
    states = torch.from_numpy(raw.view(np.uint8).reshape(-1)).cuda()
    sim.rng_pos = 7
    got = TT.run_tracks(chain, tracks, states)
    TT.assert_tracks(got, want, what="1100 tracks")
    assert sim.rng_pos == pos
    got_states = states.cpu().numpy().view(np.uint64).reshape(n, 31)
    exp_states = np.array([list(A.state_bits(s[0])) + [s[1]] for _, s in want], np.uint64)
    assert (got_states == exp_states).all(), "states of tracks %s" % np.nonzero((got_states != exp_states).any(axis=1))[0][:10]
    assert [s[0] for s in chain.track_stats(n)] == [(f + 15) // 16 for f in frames]


# ---------------------------------------------------------------------------------------------- B3
def test_hiss_windows_at_the_step_jump_boundary(sim):
    ap = T.PRESETS["mono_lp"]()
    assert ap.hiss_level != 0 and ap.channels == 1
    blocks = M.boundary_blocks()
    a = A.make_input("music", 140000, 1, 75)
    want, st, pos = A.run_checker(ap, a, rng_pos=3, block="blocks=" + A.block_spec(blocks))
    chain = ntscsim.AudioChain(ap, sim=sim)
    sim.rng_pos = 3
    got = TA.run_device(chain, a, blocks)
    TA.assert_same(chain, got, want, st, "boundary blocks")
    assert sim.rng_pos == pos
    assert chain.stats()[0] == (140000 + 4095) // 4096


# ---------------------------------------------------------------------------------------------- B4
@pytest.mark.parametrize("frames,count0", [((1 << 18) - 1, 0), (1 << 18, 3000000000), ((1 << 18) + 3, 0)], ids=["2p18-1", "2p18_count_3e9", "2p18+3"])
def test_sin_fill_at_the_split(sim, frames, count0):
    """2^18 + 3 frames make four parts of 65537, 65537, 65537 and 65534: a wrong part offset or length changes bytes."""
    cp = _capi.make_cass_params(["-preset", "3"])
    assert cp.taps == 57 and cp.head_tilt_waver != 0
    a = A.make_input("music", frames, 2, 76)
    want, st, pos = CR.run_checker(cp, a, count0=count0, rng_pos=3)
    chain = ntscsim.Cassette(cp, sim=sim)
    chain.state = (tuple([0.0] * 28), count0, ())
    sim.rng_pos = 3
    got = TC.run_device(chain, a)
    TC.assert_same(chain, got, want, st, "%d frames from %d" % (frames, count0))
    assert sim.rng_pos == pos
    assert chain.stats()[0] == (frames + 4095) // 4096


# ---------------------------------------------------------------------------------------------- B5
def test_pulses_past_65535_workgroups(sim):
    """One linear mono call of 65535 * 256 + 300 frames: the last 300 frames are the second trip of the first 300
    lanes of k_audio_pulses.  The input is a short signal tiled; hiss is off to keep the planes small."""
    ap = TA.params(["-vhs", "-vhs-hifi", "0", "-audio-hiss", "-200"])
    assert ap.channels == 1 and ap.hiss_level == 0 and ap.buzz != 0
    frames = 65535 * 256 + 300
    short = A.make_input("music", 30011, 1, 77)
    a = np.ascontiguousarray(np.tile(short, (frames // len(short) + 1, 1))[:frames])
    want, st, pos = A.run_checker(ap, a, rng_pos=3)
    chain = ntscsim.AudioChain(ap, sim=sim)
    sim.rng_pos = 3
    got = TA.run_device(chain, a)
    TA.assert_same(chain, got, want, st, "%d frames" % frames)
    assert sim.rng_pos == pos == 3
    assert chain.stats()[0] == (frames + 4095) // 4096


# ---------------------------------------------------------------------------------------------- B6
def test_mixed_repairs_in_the_audio_chain(sim):
    ap, a = M.mixed_audio_case()
    W, p0 = M.MIXED_AUDIO["warmup"], M.MIXED_AUDIO["rng_pos"]
    plan_stats, which = A.plan(ap, a, M.MIXED_SEG, W, rng_pos=p0)
    assert A.mixed_repairs(plan_stats[0], which), which
    want, st, pos = A.run_checker(ap, a, rng_pos=p0)
    chain = ntscsim.AudioChain(ap, sim=sim)
    chain.set_plan(M.MIXED_SEG, W)
    sim.rng_pos = p0
    got = TA.run_device(chain, a)
    TA.assert_same(chain, got, want, st, "repaired %s" % which)
    assert sim.rng_pos == pos
    assert chain.stats() == plan_stats


def test_mixed_repairs_in_the_cassette(sim):
    cp, a = M.mixed_cass_case()
    wf, wb, p0 = M.MIXED_CASS["front"], M.MIXED_CASS["back"], M.MIXED_CASS["rng_pos"]
    plan_stats, front, back = CR.plan(cp, a, M.MIXED_SEG, wf, wb, rng_pos=p0)
    assert A.mixed_repairs(plan_stats[0], front) and A.mixed_repairs(plan_stats[0], back), (front, back)
    want, st, pos = CR.run_checker(cp, a, rng_pos=p0)
    chain = ntscsim.Cassette(cp, sim=sim)
    chain.set_plan(M.MIXED_SEG, wf, wb)
    sim.rng_pos = p0
    got = TC.run_device(chain, a)
    TC.assert_same(chain, got, want, st, "front repaired %s, back %s" % (front, back))
    assert sim.rng_pos == pos
    assert chain.stats() == plan_stats


def test_mixed_repairs_in_one_track_of_three(sim):
    ap, tracks, first = M.mixed_tracks_case()
    W = M.MIXED_TRACKS["warmup"]
    plans = [A.plan(ap, t, M.MIXED_SEG, W, rng_pos=p) for t, p in zip(tracks, first)]
    assert plans[0][0][1] == 0 and plans[2][0][1] == 0 and A.mixed_repairs(plans[1][0][0], plans[1][1]), plans
    want, pos = A.run_tracks_checker(ap, tracks, pos=first[0])
    chain = ntscsim.AudioChain(ap, sim=sim)
    chain.set_plan(M.MIXED_SEG, W)
    states = chain.zero_states(3)
    sim.rng_pos = first[0]
    got = TT.run_tracks(chain, tracks, states)
    TT.assert_tracks(got, want, states, what="repaired %s" % plans[1][1])
    assert sim.rng_pos == pos
    assert chain.track_stats(3) == [p[0] for p in plans]
