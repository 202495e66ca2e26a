"""Many independent audio tracks in one call (ntscsim_audio_tracks_device: k_audio_hiss, k_audio_track_pulses,
k_audio_track_segments, k_audio_track_verify) against the host checker run PER TRACK (A.run_checker: the serial chain of
csrc/audio_chain.hpp, which tests/test_audio_ref.py pins to the reference's own lines), byte for byte and state bit for
state bit: the chain is exact arithmetic, so the tolerance is zero.  The expectation is never the code under test, but
for test_one_track_equals_the_existing_call, whose expectation is the existing call.

Shapes are the smallest at which the new indexing can go wrong: with plan (64, 20), tracks of 64, 1, 0, 193, 128, 385,
2 and 63 frames are 1, 1, 0, 4, 2, 7, 1 and 1 segments -- 17 in six wavefronts of three groups, groups of one wavefront
in different tracks, a track without frames between them, the last wavefront with two live groups.  The tracks are cut
back to back from one device buffer with different content in each, so that a warm-up that crossed a track boundary
would change bits.  60,000 / 12,000 frames are the smallest with speculation inside a track at the default plan."""
import ctypes as C

import numpy as np
import pytest

import _audio_ref as A
import _audio_tracks as T
import ntscsim
from ntscsim import _capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sim():
    s = ntscsim.FieldSimulator(device=0)
    yield s
    s.close()


def spec_of(blocks):
    return "blocks=" + ",".join("%d:%s" % (n, "a" if p is None else p) for n, p in blocks)


def expect(ap, tracks, counts=None, pos=0, blocks=None):
    """The checker per track, in order, the rand() position running through: ([(output, (values, count))], position)."""
    out = []
    for t, a in enumerate(tracks):
        block = spec_of(blocks[t]) if blocks is not None and blocks[t] is not None else 0
        if len(a) == 0:
            out.append((a, (tuple([0.0] * 30), counts[t] if counts else 0)))
            for _n, p in (blocks[t] if blocks is not None and blocks[t] is not None else []):
                pos = pos if p is None else p                                   # a block without samples still sets the position
            continue
        want, st, pos = A.run_checker(ap, a, count0=counts[t] if counts else 0, rng_pos=pos, block=block)
        out.append((want, st))
    return out, pos


def run_tracks(chain, tracks, states=None, blocks=None):
    """The tracks back to back in one device buffer, through one tracks call: the outputs as numpy arrays."""
    import torch
    ch = chain.channels
    frames = [len(a) for a in tracks]
    whole = np.concatenate([np.ascontiguousarray(a).reshape(-1, ch) for a in tracks]) if tracks else np.zeros((0, ch), np.int16)
    src = torch.from_numpy(whole).cuda()
    dst = torch.full_like(src, 0x5555)
    chain.process_tracks(T.cut(src, frames), T.cut(dst, frames), states, blocks)
    chain.sync()
    assert torch.equal(src.cpu(), torch.from_numpy(whole)), "the call wrote its source"
    return [np.array(x) for x in T.cut(dst.cpu().numpy(), frames)]


def assert_tracks(got, want, states=None, slots=None, what=""):
    for t, (g, (w, st)) in enumerate(zip(got, want)):
        bad = int((g != w).sum())
        first = int(np.argmax((g != w).reshape(-1))) if bad else -1
        assert bad == 0, "%s track %d: %d wrong samples, first at %d" % (what, t, bad, first)
        slot = t if slots is None else slots[t]
        if states is not None and slot is not None:
            vals, count = ntscsim.AudioChain.track_state(states, slot)
            assert count == st[1], "%s track %d" % (what, t)
            assert (A.state_bits(vals) == A.state_bits(st[0])).all(), "%s track %d" % (what, t)


def test_the_feature_exists(sim):
    """Two stereo tracks of 4096 frames at the default preset equal the checker per track."""
    ap = T.PRESETS["stereo_hifi"]()
    tracks = T.cut(T.make_tracks([4096, 4096], 2, seed=21), [4096, 4096])
    want, pos = expect(ap, tracks)
    sim.rng_pos = 0
    chain = ntscsim.AudioChain(ap, sim=sim)
    states = chain.zero_states(2)
    got = run_tracks(chain, tracks, states)
    assert_tracks(got, want, states)
    assert sim.rng_pos == pos == 2 * 8192


@pytest.mark.parametrize("preset", ["mono_lp", "stereo_hifi", "stereo_linear"])
def test_groups_straddle_tracks(sim, preset):
    ap = T.PRESETS[preset]()
    chain = ntscsim.AudioChain(ap, sim=sim)
    for plan, frames in (((64, 20), T.STRADDLE), ((1, 0), T.STRADDLE[:4]), ((65, 64), T.STRADDLE[:4])):
        tracks = T.cut(T.make_tracks(frames, ap.channels), frames)
        want, pos = expect(ap, tracks, pos=3)
        chain.set_plan(*plan)
        sim.rng_pos = 3
        states = chain.zero_states(len(frames))
        got = run_tracks(chain, tracks, states)
        assert_tracks(got, want, states, what="plan %s" % (plan,))
        assert sim.rng_pos == pos
        stats = chain.track_stats(len(frames))
        assert [s[0] for s in stats] == [(f + plan[0] - 1) // plan[0] for f in frames], plan
    chain.set_plan(0, 0)


@pytest.mark.parametrize("preset,frames", [("stereo_hifi", 60000), ("stereo_linear", 12000)])
def test_default_plan_speculates_inside_a_track(sim, preset, frames):
    """Zero repairs is a condition on these inputs, shown on the CPU by tests/test_audio_tracks_host.py
    (test_default_plan_sets_need_no_repair runs the same generator inputs through the same plan)."""
    ap = T.PRESETS[preset]()
    tracks = T.cut(T.make_tracks([frames] * 3, 2), [frames] * 3)
    want, pos = expect(ap, tracks, pos=1000)
    sim.rng_pos = 1000
    chain = ntscsim.AudioChain(ap, sim=sim)
    assert (frames + 4095) // 4096 * 4096 > chain.default_warmup() + 4096      # a segment past a whole warm-up, in every track
    states = chain.zero_states(3)
    got = run_tracks(chain, tracks, states)
    assert_tracks(got, want, states)
    assert sim.rng_pos == pos
    assert chain.track_stats(3) == [((frames + 4095) // 4096, 0)] * 3


def test_repair_in_some_tracks_only(sim):
    ap = T.PRESETS["no_hiss"]()
    assert ap.hiss_level == 0
    tracks = T.cut(T.make_tracks([3000, 3000], 2, ["music", "silence"]), [3000, 3000])
    want, _ = expect(ap, tracks)
    chain = ntscsim.AudioChain(ap, sim=sim)
    chain.set_plan(256, 0)
    states = chain.zero_states(2)
    got = run_tracks(chain, tracks, states)
    assert_tracks(got, want, states)
    assert not got[1].any()
    assert chain.track_stats(2) == [(12, 11), (12, 0)]                          # silence without hiss: a zero state IS the true state


def ctx_state_bytes(sim):
    s = _capi.AudioState()
    assert sim._lib.ntscsim_audio_get_state(sim._h, C.byref(s)) == _capi.OK
    return bytes(s)


def test_states_and_counts(sim):
    """A NULL state, a state at a count of hours (linear: the buzz depends on it), a state a previous tracks call left;
    a prefix call and then the rest on the same state tensor equal the checker on the whole tracks.  The ctx's own
    state is not touched."""
    ap = T.PRESETS["stereo_linear"]()
    n_, b_, c_ = T.cut(T.make_tracks([3000, 3000, 3000], 2, ["music", "quiet", "music"], seed=9), [3000] * 3)
    chain = ntscsim.AudioChain(ap, sim=sim)
    chain.set_plan(256, 64)
    run_tracks(chain, [c_[:500]])                                               # not a tracks concern: make the ctx's state something
    import torch
    src = torch.from_numpy(np.ascontiguousarray(b_[:700])).cuda()
    chain.process(src, torch.zeros_like(src))
    chain.sync()
    before = ctx_state_bytes(sim)
    assert any(before)
    p0 = 17
    # draws in call order: n_ whole, b_[:1100], c_[:700]; then b_[1100:], c_[700:]
    pb1, pc1 = p0 + 6000, p0 + 6000 + 2200
    pb2 = pc1 + 1400
    pc2 = pb2 + 3800
    want, _ = expect(ap, [n_, b_, c_], counts=[0, 3000000000, 0], pos=p0,
                     blocks=[None, [(1100, pb1), (1900, pb2)], [(700, pc1), (2300, pc2)]])
    states = chain.zero_states(2)
    chain.set_track_state(states, 0, (tuple([0.0] * 30), 3000000000))
    assert chain.track_state(states, 0) == (tuple([0.0] * 30), 3000000000)
    sim.rng_pos = p0
    # process_tracks gives every track a state slot or none at all: the mixed call goes through the C ABI
    got1 = run_tracks_abi(sim, chain, [n_, b_[:1100], c_[:700]], states, [None, 0, 1])
    assert sim.rng_pos == pb2
    got2 = run_tracks(chain, [b_[1100:], c_[700:]], states)
    assert sim.rng_pos == pc2 + 4600
    got = [got1[0], np.concatenate([got1[1], got2[0]]), np.concatenate([got1[2], got2[1]])]
    assert_tracks(got, want, states, slots=[None, 0, 1])
    assert ctx_state_bytes(sim) == before
    chain.set_plan(0, 0)


def run_tracks_abi(sim, chain, tracks, states, slots):
    """as run_tracks, with track t on state slot slots[t] (None: a NULL state)"""
    import torch
    ch = chain.channels
    frames = [len(a) for a in tracks]
    whole = np.concatenate([np.ascontiguousarray(a).reshape(-1, ch) for a in tracks])
    src = torch.from_numpy(whole).cuda()
    dst = torch.full_like(src, 0x5555)
    arr = (_capi.AudioTrack * len(tracks))()
    descs = (_capi.AudioDesc * len(tracks))()
    at = 0
    for t, f in enumerate(frames):
        descs[t].src, descs[t].dst = src.data_ptr() + at * ch * 2, dst.data_ptr() + at * ch * 2
        descs[t].samples, descs[t].rng_pos = f, _capi.RNG_AUTO
        arr[t].blocks = C.cast(C.byref(descs[t]), C.POINTER(_capi.AudioDesc))
        arr[t].n_blocks = 1
        arr[t].state = None if slots[t] is None else states.data_ptr() + slots[t] * chain.STATE_BYTES
        at += f
    assert sim._lib.ntscsim_audio_tracks_device(sim._h, arr, len(tracks), C.c_void_p(sim._torch_stream())) == _capi.OK
    sim.sync()
    assert torch.equal(src.cpu(), torch.from_numpy(whole)), "the call wrote its source"
    return [np.array(x) for x in T.cut(dst.cpu().numpy(), frames)]


def test_rand_positions(sim):
    ap = T.params(["-vhs", "-vhs-hifi", "0"])                                   # mono, hiss level 39
    assert ap.hiss_level != 0 and ap.channels == 1
    frames = [500, 700, 300]
    tracks = T.cut(T.make_tracks(frames, 1, seed=70), frames)
    chain = ntscsim.AudioChain(ap, sim=sim)
    chain.set_plan(128, 32)
    # explicit positions that go backwards from track to track
    blocks = [[(500, 5000)], [(700, 3000)], [(300, 1000)]]
    want, pos = expect(ap, tracks, blocks=blocks)
    sim.rng_pos = 99
    states = chain.zero_states(3)
    got = run_tracks(chain, tracks, states, blocks)
    assert_tracks(got, want, states, what="explicit")
    assert sim.rng_pos == pos == 1300
    # NTSCSIM_RNG_AUTO throughout: the position moves by the channel-samples
    want, pos = expect(ap, tracks, pos=1 << 33)
    sim.rng_pos = 1 << 33
    states = chain.zero_states(3)
    got = run_tracks(chain, tracks, states)
    assert_tracks(got, want, states, what="auto")
    assert sim.rng_pos == pos == (1 << 33) + sum(frames)
    # several blocks per track, empty ones among them, one block's position set in mid-track
    blocks = [[(200, None), (0, None), (300, None)], [(1, None), (699, 77777)], [(0, 12), (300, None), (0, None)]]
    want, pos = expect(ap, tracks, pos=41, blocks=blocks)
    sim.rng_pos = 41
    states = chain.zero_states(3)
    got = run_tracks(chain, tracks, states, blocks)
    assert_tracks(got, want, states, what="mixed")
    assert sim.rng_pos == pos == 12 + 300
    chain.set_plan(0, 0)


def test_one_track_equals_the_existing_call(sim):
    import torch
    ap = T.params(["-vhs", "-vhs-hifi", "0"])
    a = A.make_input("music", 9000, 1, 8)
    blocks = [(1500, 700), (0, 5), (1, 100000), (2999, None), (1700, 12), (800, 12), (2000, 1 << 33)]
    chain = ntscsim.AudioChain(ap, sim=sim)
    src = torch.from_numpy(a).cuda()
    dst = torch.full_like(src, 0x5555)
    sim.rng_pos = 1
    chain.process(src, dst, blocks)
    chain.sync()
    one, one_state, one_pos = dst.cpu().numpy(), chain.state, sim.rng_pos
    sim.rng_pos = 1
    states = chain.zero_states(1)
    got = run_tracks(chain, [a], states, [blocks])
    assert (got[0] == one).all()
    vals, count = chain.track_state(states, 0)
    assert count == one_state[1] and (A.state_bits(vals) == A.state_bits(one_state[0])).all()
    assert sim.rng_pos == one_pos
    assert chain.track_stats(1) == [chain.stats()]


def test_many_tracks(sim):
    """200 mono tracks of 100 frames, each with its own state and sample count"""
    ap = T.PRESETS["mono_lp"]()
    frames = [100] * 200
    counts = [1000 * t for t in range(200)]
    tracks = T.cut(T.make_tracks(frames, 1, seed=5), frames)
    want, pos = expect(ap, tracks, counts=counts, pos=7)
    chain = ntscsim.AudioChain(ap, sim=sim)
    states = chain.zero_states(200)
    for t in range(200):
        chain.set_track_state(states, t, (tuple([0.0] * 30), counts[t]))
    sim.rng_pos = 7
    got = run_tracks(chain, tracks, states)
    assert_tracks(got, want, states)
    assert sim.rng_pos == pos
    assert chain.track_stats(200) == [(1, 0)] * 200


def test_nocomp(sim):
    import torch
    ap = T.PRESETS["nocomp"]()
    frames = [100, 0, 300]
    tracks = T.cut(T.make_tracks(frames, ap.channels), frames)
    chain = ntscsim.AudioChain(ap, sim=sim)
    states = torch.arange(3 * chain.STATE_BYTES, dtype=torch.int32).to(torch.uint8).cuda()
    keep = states.clone()
    sim.rng_pos = 9
    got = run_tracks(chain, tracks, states)
    for g, a in zip(got, tracks):
        assert (g == a).all()
    assert torch.equal(states, keep)
    assert sim.rng_pos == 9
    assert chain.track_stats(3) == [(0, 0)] * 3


def test_error_codes(sim):
    import torch
    lib = sim._lib
    ap = T.PRESETS["stereo_hifi"]()
    one = (_capi.AudioTrack * 1)()
    fresh = ntscsim.FieldSimulator(device=0)
    try:
        assert lib.ntscsim_audio_tracks_device(fresh._h, one, 1, None) == _capi.E_ARG           # no bind
    finally:
        fresh.close()
    chain = ntscsim.AudioChain(ap, sim=sim)
    buf = torch.zeros(8192, dtype=torch.int16, device="cuda")
    out = torch.full((8192,), 0x5555, dtype=torch.int16, device="cuda")
    states = chain.zero_states(3)
    base, obase, sbase = buf.data_ptr(), out.data_ptr(), states.data_ptr()
    assert sbase % 8 == 0
    sim.rng_pos = 5

    def call(t0, t1=None, n=None):
        """tracks given as (src, dst, samples, state)"""
        given = [t for t in (t0, t1) if t is not None]
        arr = (_capi.AudioTrack * len(given))()
        descs = (_capi.AudioDesc * len(given))()
        for t, (src, dst, samples, state) in enumerate(given):
            descs[t].src, descs[t].dst, descs[t].samples, descs[t].rng_pos = src, dst, samples, _capi.RNG_AUTO
            arr[t].blocks = C.cast(C.byref(descs[t]), C.POINTER(_capi.AudioDesc))
            arr[t].n_blocks = 1
            arr[t].state = state
        return lib.ntscsim_audio_tracks_device(sim._h, arr, len(given) if n is None else n, None)

    ok0, ok1 = (base, obase, 100, sbase), (base + 4096, obase + 4096, 100, sbase + chain.STATE_BYTES)
    assert lib.ntscsim_audio_tracks_device(None, one, 1, None) == _capi.E_ARG                   # a NULL ctx
    assert call(ok0, ok1, n=-1) == _capi.E_ARG
    assert lib.ntscsim_audio_tracks_device(sim._h, None, 1, None) == _capi.E_ARG                # NULL tracks
    nb = (_capi.AudioTrack * 1)()
    nb[0].n_blocks = 1
    assert lib.ntscsim_audio_tracks_device(sim._h, nb, 1, None) == _capi.E_ARG                  # NULL blocks
    assert call(ok0, (None, obase + 4096, 100, None)) == _capi.E_ARG                            # NULL and odd pointers
    assert call(ok0, (base + 4096, None, 100, None)) == _capi.E_ARG
    assert call(ok0, (base + 4097, obase + 4096, 100, None)) == _capi.E_ARG
    assert call(ok0, (base + 4096, obase + 4097, 100, None)) == _capi.E_ARG
    assert call(ok0, (base + 4096, obase + 4096, 100, sbase + chain.STATE_BYTES + 4)) == _capi.E_ARG   # a state not 8-byte aligned
    assert call(ok0, (base + 4096, obase + 4096, 100, sbase)) == _capi.E_ARG                    # two tracks, one state
    assert call(ok0, (base + 4096, obase + 4096, 100, sbase + 240)) == _capi.E_ARG              # overlapping states
    assert call((base, base, 100, sbase)) == _capi.E_ARG                                        # in place
    assert call((base, base + 396, 100, sbase)) == _capi.E_ARG                                  # dst overlaps the end of its src
    assert call(ok0, (base + 4096, base + 396, 100, None)) == _capi.E_ARG                       # dst overlaps the src of another track
    assert call((base + 4096, base + 396, 100, None), ok0) == _capi.E_ARG
    sim.sync()
    assert sim.rng_pos == 5                                                                     # a refused call draws nothing
    assert bool((out == 0x5555).all()) and not bool(buf.any()) and not bool(states.any())       # and writes nothing
    assert lib.ntscsim_audio_debug_track_stats(sim._h, None, 1) == _capi.E_ARG
    assert call(ok0, (None, None, 0, None)) == _capi.OK                                         # an empty block needs no pointers
    assert lib.ntscsim_audio_tracks_device(sim._h, None, 0, None) == _capi.OK                   # no tracks at all
    assert call(ok0, ok1) == _capi.OK
    sim.sync()
    assert sim.rng_pos == 5 + 200 + 400
    s = (_capi.AudioStats * 3)()
    assert lib.ntscsim_audio_debug_track_stats(sim._h, s, 3) == _capi.E_ARG                     # the last call had two tracks
    assert lib.ntscsim_audio_debug_track_stats(sim._h, s, 2) == _capi.OK


def test_the_veneer(sim):
    """process_tracks on tensors of unequal length that are not neighbours, track_stats, the state helpers"""
    import torch
    ap = T.PRESETS["stereo_hifi"]()
    frames = [700, 0, 129, 2000]
    tracks = T.cut(T.make_tracks(frames, 2, seed=90), frames)
    want, pos = expect(ap, tracks, pos=2)
    chain = ntscsim.AudioChain(ap, sim=sim)
    chain.set_plan(128, 40)
    srcs = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in tracks]
    dsts = [torch.full_like(s, 0x5555) for s in srcs]
    states = chain.zero_states(4)
    assert states.dtype == torch.uint8 and states.numel() == 4 * 248 and chain.STATE_BYTES == 248
    assert chain.track_state(states, 3) == (tuple([0.0] * 30), 0)
    sim.rng_pos = 2
    chain.process_tracks(srcs, dsts, states)
    chain.sync()
    assert_tracks([d.cpu().numpy() for d in dsts], want, states)
    assert sim.rng_pos == pos
    assert [s[0] for s in chain.track_stats(4)] == [6, 0, 2, 16]
    assert chain.track_state(states, 1) == (tuple([0.0] * 30), 0)               # a track without frames leaves its state
    # states=None: every track from zeros, nothing kept
    dsts2 = [torch.full_like(s, 0x5555) for s in srcs]
    sim.rng_pos = 2
    chain.process_tracks(srcs, dsts2)
    chain.sync()
    assert_tracks([d.cpu().numpy() for d in dsts2], want)
    # the mirror has the header's layout
    assert C.sizeof(_capi.AudioTrack) == 24 and _capi.AudioTrack.state.offset == 16 and _capi.AudioTrack.n_blocks.offset == 8
    chain.set_plan(0, 0)
