"""Many independent cassette tracks in one call (ntscsim_cass_tracks_device: k_audio_hiss, k_cass_track_front,
k_cass_track_front_verify, k_cass_track_conv, k_cass_track_back, k_cass_track_back_verify) against the serial chain of
csrc/cass_chain.hpp run PER TRACK from that track's state and count, with every tap of the FIR and this host's sines
(tests/cass_tracks_check.cpp `expect`, one process per track set; tests/test_cass_tracks_host.py pins that mode to
tests/cass_chain_check.cpp, which tests/test_cass_ref.py pins to the reference's own lines).  The chain is exact
arithmetic, so the tolerance is zero: output bytes, and the whole state byte for byte -- the 28 filter values, the
count, the taps, the taps - 1 history frames, and the rest of the history, which must stay as it came.  The ctx's rand()
position is compared as well.  The expectation is never the code under test, but for
test_one_track_equals_the_existing_call, whose expectation is the existing call.

Shapes are the smallest at which the new indexing can go wrong (tests/_cass_tracks.py).  The tracks are cut back to back
from one device buffer with different content in each, so that a warm-up, a halo or a tile that crossed a track boundary
would change bits; the destination is pre-filled with a pattern and the source is compared afterwards.

The cassette parameters have no `enabled`: there is no copying mode to test."""
import ctypes as C

import numpy as np
import pytest

import _cass_ref as A
import _cass_tracks as T
import ntscsim
from ntscsim import _capi

pytestmark = pytest.mark.gpu
SB = T.STATE_BYTES


@pytest.fixture(scope="module")
def sim():
    s = ntscsim.FieldSimulator(device=0)
    yield s
    s.close()


def state_tensor(raw):
    import torch
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()


def launch(sim, chain, src, dst, frames, counts, states, slots=None, stream=None):
    """One tracks call over tracks cut back to back from src / dst.  slots: None (track t on state t of `states`, through
    the veneer) or per track a state index or None for a NULL state (through the C ABI).  Does not synchronise."""
    if slots is None:
        chain.process_tracks(T.cut(src, frames), T.cut(dst, frames), counts, states, stream=stream)
        return
    n = len(frames)
    arr = (_capi.CassTrack * n)()
    descs = (_capi.CassDesc * n)()
    at = 0
    for t, f in enumerate(frames):
        descs[t].src, descs[t].dst = src.data_ptr() + at * 4, dst.data_ptr() + at * 4
        descs[t].samples, descs[t].rng_pos = f, _capi.RNG_AUTO
        arr[t].blocks = C.cast(C.byref(descs[t]), C.POINTER(_capi.CassDesc))
        arr[t].n_blocks = 1
        arr[t].count = counts[t]
        arr[t].state = None if slots[t] is None else states.data_ptr() + slots[t] * SB
        at += f
    assert sim._lib.ntscsim_cass_tracks_device(sim._h, arr, n, C.c_void_p(stream if stream is not None else sim._torch_stream())) == _capi.OK


def run_tracks(sim, chain, whole, frames, counts, states, slots=None):
    """The tracks of `whole` ([sum(frames), 2]) through one tracks call: the outputs cut per track."""
    import torch
    src = torch.from_numpy(np.ascontiguousarray(whole)).cuda()
    dst = torch.full_like(src, 0x5555)
    launch(sim, chain, src, dst, frames, counts, states, slots)
    chain.sync()
    assert torch.equal(src.cpu(), torch.from_numpy(np.ascontiguousarray(whole))), "the call wrote its source"
    return T.cut(dst.cpu().numpy(), frames)


def assert_tracks(got, want, states=None, want_states=None, skip=(), what=""):
    for t, (g, w) in enumerate(zip(got, want)):
        bad = int((g != w).sum())
        first = int(np.argmax((g != w).reshape(-1))) if bad else -1
        assert bad == 0, "%s track %d: %d wrong samples, first at %d" % (what, t, bad, first)
    if states is not None:
        raw = states.cpu().numpy().tobytes()
        for t in range(len(raw) // SB):
            if t in skip:
                continue
            a, b = raw[t * SB:(t + 1) * SB], want_states[t * SB:(t + 1) * SB]
            if a != b:
                x, y = _capi.CassState.from_buffer_copy(a), _capi.CassState.from_buffer_copy(b)
                diff = [i for i in range(0, SB, 8) if a[i:i + 8] != b[i:i + 8]]
                raise AssertionError("%s state %d: count %d / %d, taps %d / %d, first differing doubles at bytes %s" % (what, t, x.count, y.count, x.taps, y.taps, diff[:6]))


def test_the_feature_exists(sim):
    """Two tracks of 4096 frames at the default settings, counts 0, equal the serial chain per track."""
    cp = T.params([])
    frames, counts = [4096, 4096], [0, 0]
    a = T.make_tracks(frames, seed=21)
    want, wst, pos = T.expect(cp, a, frames, counts)
    sim.rng_pos = 0
    chain = ntscsim.Cassette(cp, sim=sim)
    states = chain.zero_states(2)
    got = run_tracks(sim, chain, a, frames, counts, states)
    assert_tracks(got, want, states, wst)
    assert sim.rng_pos == pos == 4 * 4096
    assert chain.track_stats(2) == [(1, 0, 0)] * 2 and chain.tilt_frames() == 4096
    assert sim.last_kernels() == ["k_audio_hiss", "k_cass_track_front", "k_cass_track_front_verify", "k_cass_track_conv"]


@pytest.mark.parametrize("flags", T.STRADDLE_FLAGS, ids=lambda f: " ".join(f) or "default")
def test_groups_straddle_tracks(sim, flags):
    cp = T.params(flags)
    assert cp.taps == (57 if "-preset" in flags else 8)
    chain = ntscsim.Cassette(cp, sim=sim)
    for plan, frames in T.STRADDLE_PLANS:
        counts = [0] * len(frames)
        a = T.make_tracks(frames)
        want, wst, pos = T.expect(cp, a, frames, counts, rng_pos=3)
        chain.set_plan(*plan)
        sim.rng_pos = 3
        states = chain.zero_states(len(frames))
        got = run_tracks(sim, chain, a, frames, counts, states)
        assert_tracks(got, want, states, wst, what="plan %s" % (plan,))
        assert sim.rng_pos == pos
        stats = chain.track_stats(len(frames))
        assert [s[0] for s in stats] == [(f + plan[0] - 1) // plan[0] for f in frames], plan
        assert chain.tilt_frames() == max(frames)
    chain.set_plan(0, 0, 0)


@pytest.mark.parametrize("flags", [A.BAD_DECK, A.BAD_DECK + ["-deemphasis", "1"]], ids=" ".join)
def test_tiles(sim, flags):
    """The tile edges, a one-frame last tile, three tiles in one track, a track without frames; every track starts from
    the non-zero history that the serial chain leaves behind a 100-frame lead-in, set through set_track_state."""
    cp = T.params(flags)
    assert cp.taps == 57
    n = len(T.TILES)
    counts = [0, 1000, 5, 77, 100000]
    lead = T.make_tracks([100] * n, seed=77)
    _, lead_states, _ = T.expect(cp, lead, [100] * n, counts)
    chain = ntscsim.Cassette(cp, sim=sim)
    states = chain.zero_states(n)
    for t in range(n):
        s = _capi.CassState.from_buffer_copy(lead_states[t * SB:(t + 1) * SB])
        assert s.count == counts[t] + 100 and any(s.history[k][0] != 0.0 for k in range(56))
        vals = [x for c in s.bandpass for x in c] + list(s.pre) + list(s.post)
        chain.set_track_state(states, t, (vals, s.count, [(s.history[k][0], s.history[k][1]) for k in range(56)]))
        assert chain.track_state(states, t)[1] == s.count
    assert states.cpu().numpy().tobytes() == lead_states
    counts = [c + 100 for c in counts]
    a = T.make_tracks(T.TILES)
    want, wst, pos = T.expect(cp, a, T.TILES, counts, states_in=lead_states, rng_pos=9)
    sim.rng_pos = 9
    got = run_tracks(sim, chain, a, T.TILES, counts, states)
    assert_tracks(got, want, states, wst)
    assert sim.rng_pos == pos
    assert wst[3 * SB:4 * SB] == lead_states[3 * SB:4 * SB]                     # the track without frames: as it came
    assert [s[0] for s in chain.track_stats(n)] == [1, 1, 1, 0, 1]


def test_counts_and_the_tilt_union(sim):
    import torch
    cp = T.params([])
    chain = ntscsim.Cassette(cp, sim=sim)
    frames, counts = [300] * 16, [0] * 16
    a = T.make_tracks(frames)
    want, wst, pos = T.expect(cp, a, frames, counts, rng_pos=5)
    sim.rng_pos = 5
    states = chain.zero_states(16)
    got = run_tracks(sim, chain, a, frames, counts, states)
    assert_tracks(got, want, states, wst, what="16 at count 0")
    assert sim.rng_pos == pos and chain.tilt_frames() == 300
    # partial overlaps and a range far away; track 2 has a NULL state; count and taps are garbage on entry
    frames, counts = list(T.UNION_FRAMES), list(T.UNION_COUNTS)
    a = T.make_tracks(frames, seed=50)
    raw = bytearray(5 * SB)
    for t in range(5):
        s = _capi.CassState.from_buffer(raw, t * SB)
        s.count, s.taps = 0xDEADBEEF00 + t, 4000 + t
    want, wst, pos = T.expect(cp, a, frames, counts, states_in=bytes(raw), null=(2,), rng_pos=5)
    states = state_tensor(raw)
    sim.rng_pos = 5
    got = run_tracks(sim, chain, a, frames, counts, states, slots=[0, 1, None, 3, 4])
    assert_tracks(got, want, states, wst, what="union")
    assert wst[2 * SB:3 * SB] == bytes(raw[2 * SB:3 * SB])                      # the slot no track used: untouched
    assert sim.rng_pos == pos and chain.tilt_frames() == 750
    for t in (0, 1, 3, 4):
        _vals, count, _hist = chain.track_state(states, t)
        assert count == counts[t] + frames[t]
    assert int(states.view(torch.uint8)[4 * SB + 232:4 * SB + 236].cpu().numpy().view(np.uint32)[0]) == 8   # taps
    # the far track's tilt is its own count's: it differs from a run of the same input at count 0
    z, _, _ = T.expect(cp, a, frames, [0] * 5, null=(2,), rng_pos=5)
    assert int((z[4] != want[4]).sum()) > 0


def test_repairs_in_some_tracks_only(sim):
    cp = T.params(T.NO_HISS_DEEMPH)
    assert cp.hiss_level == 0
    frames, counts = [3000, 3000], [0, 0]
    a = T.make_tracks(frames, ["music", "silence"])
    want, wst, _ = T.expect(cp, a, frames, counts)
    host_stats, _, _ = T.run_check(cp, a, frames, counts, (256, 0, 0))
    chain = ntscsim.Cassette(cp, sim=sim)
    chain.set_plan(256, 0, 0)
    states = chain.zero_states(2)
    got = run_tracks(sim, chain, a, frames, counts, states)
    assert_tracks(got, want, states, wst)
    assert not got[1].any()
    stats = chain.track_stats(2)
    assert stats == host_stats and stats[1] == (12, 0, 0) and stats[0][1] == 11 and stats[0][2] > 0
    chain.set_plan(0, 0, 0)


def test_default_plan_speculates_inside_a_track(sim):
    """-high 100: the front's warm-up is 5056 frames, so the third segment of every track starts from zeros a whole
    warm-up early (tests/test_cass_gpu.py).  The repair counts are the host plan's."""
    cp = T.params(T.HIGH100)
    frames, counts = [12000] * 3, [0, 44100, 7]
    a = T.make_tracks(frames)
    want, wst, pos = T.expect(cp, a, frames, counts, rng_pos=1000)
    host_stats, _, _ = T.run_check(cp, a, frames, counts, (4096, -1, -1), rng_pos=1000)
    sim.rng_pos = 1000
    chain = ntscsim.Cassette(cp, sim=sim)
    wf, _wb = chain.default_warmups()
    assert wf == 5056 and 3 * 4096 > wf + 4096
    states = chain.zero_states(3)
    got = run_tracks(sim, chain, a, frames, counts, states)
    assert_tracks(got, want, states, wst)
    assert sim.rng_pos == pos
    assert chain.track_stats(3) == host_stats == [(3, 0, 0)] * 3
    assert sim.last_kernels() == ["k_audio_hiss", "k_cass_track_front", "k_cass_track_front_verify", "k_cass_track_conv", "k_cass_track_back",
                                  "k_cass_track_back_verify"]


def test_one_track_equals_the_existing_call(sim):
    import torch
    cp = T.params(["-preset", "0", "-preemphasis", "1", "-deemphasis", "1"])     # 25 taps
    a = A.make_input("music", 9000, 2, 8)
    blocks = [(1500, 700), (0, 5), (1, 100000), (2999, None), (1700, 12), (800, 12), (2000, 1 << 33)]
    chain = ntscsim.Cassette(cp, sim=sim)
    chain.debug_time_kernels(True)
    src = torch.from_numpy(a).cuda()
    dst = torch.full_like(src, 0x5555)
    chain.state = (tuple([0.0] * 28), 12345, ())
    sim.rng_pos = 1
    chain.process(src, dst, blocks)
    chain.sync()
    one, one_state, one_pos, one_stats = dst.cpu().numpy(), chain.state, sim.rng_pos, chain.stats()
    assert chain.tilt_frames() == 9000
    sim.rng_pos = 1
    states = chain.zero_states(1)
    dst2 = torch.full_like(src, 0x5555)
    chain.process_tracks([src], [dst2], [12345], states, [blocks])
    chain.sync()
    assert (dst2.cpu().numpy() == one).all()
    vals, count, hist = chain.track_state(states, 0)
    assert count == one_state[1] == 12345 + 9000
    assert (np.array(vals).view(np.uint64) == np.array(one_state[0]).view(np.uint64)).all()
    assert (np.array(hist).view(np.uint64) == np.array(one_state[2]).view(np.uint64)).all()
    assert sim.rng_pos == one_pos
    assert chain.track_stats(1) == [one_stats] and chain.tilt_frames() == 9000
    ms = chain.kernel_ms()
    assert len(ms) == 8 and all(v >= 0 for v in ms) and ms[3] > 0 and ms[5] > 0 and ms[6] > 0
    chain.debug_time_kernels(False)
    assert chain.state == one_state                                             # the ctx's own state: not touched by the tracks call


def test_calls_in_flight_and_past_launch_thresholds():
    """On one stream that is not the default one, without a wait between the calls: a prefix of every track, the rest on
    the same state tensor with the counts advanced by the caller, 1100 tracks of 8 frames (more than 1024 tracks, and a
    re-make of the scratch while work is in flight), then a plain ntscsim_cass_device call, which starts from the ctx's
    own state as if no tracks call had been."""
    import torch
    cp = T.params(A.BAD_DECK + ["-deemphasis", "1"])
    frames, counts = [600, 1, 0, 193, 900], [0, 10, 20, 3000000000, 40]
    first = [f // 3 for f in frames]
    rest = [f - p for f, p in zip(frames, first)]
    a = T.make_tracks(frames, seed=60)
    a1 = np.concatenate([x[:p] for x, p in zip(T.cut(a, frames), first)])
    a2 = np.concatenate([x[p:] for x, p in zip(T.cut(a, frames), first)])
    many_f, many_c = [8] * T.MANY, [1000 * t for t in range(T.MANY)]
    am = T.make_tracks(many_f, seed=5)
    ap = A.make_input("music", 700, 2, 33)
    want1, st1, pos1 = T.expect(cp, a1, first, counts, rng_pos=2)
    counts2 = [c + p for c, p in zip(counts, first)]
    want2, st2, pos2 = T.expect(cp, a2, rest, counts2, states_in=st1, rng_pos=pos1)
    wantm, stm, posm = T.expect(cp, am, many_f, many_c, rng_pos=pos2)
    wantp, stp, posp = A.run_checker(cp, ap, rng_pos=posm)
    sim = ntscsim.FieldSimulator(device=0)
    try:
        chain = ntscsim.Cassette(cp, sim=sim)
        bufs = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (a1, a2, am, ap)]
        outs = [torch.full_like(b, 0x5555) for b in bufs]
        states, states_m = chain.zero_states(5), chain.zero_states(T.MANY)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        sim.rng_pos = 2
        launch(sim, chain, bufs[0], outs[0], first, counts, states, stream=stream.cuda_stream)
        launch(sim, chain, bufs[1], outs[1], rest, counts2, states, stream=stream.cuda_stream)
        launch(sim, chain, bufs[2], outs[2], many_f, many_c, states_m, stream=stream.cuda_stream)
        chain.process(bufs[3], outs[3], stream=stream.cuda_stream)
        assert sim.rng_pos == posp
        stream.synchronize()
        chain.sync()
        for b, x in zip(bufs, (a1, a2, am, ap)):
            assert torch.equal(b.cpu(), torch.from_numpy(np.ascontiguousarray(x))), "a call wrote its source"
        assert_tracks(T.cut(outs[0].cpu().numpy(), first), want1, what="prefix")
        assert_tracks(T.cut(outs[1].cpu().numpy(), rest), want2, states, st2, what="rest")
        assert_tracks(T.cut(outs[2].cpu().numpy(), many_f), wantm, states_m, stm, what="1100 tracks")
        assert (outs[3].cpu().numpy() == wantp).all()
        vals, count, hist = chain.state
        assert count == stp[1] == 700 and (np.array(vals).view(np.uint64) == stp[0]).all()
        assert (np.array(hist).view(np.uint64).reshape(-1, 2) == stp[2]).all()
    finally:
        sim.close()


def test_refusals(sim):
    """Every NTSCSIM_E_ARG case leaves the rand() position, the states and the destination as they were."""
    import torch
    lib = sim._lib
    cp = T.params([])
    one = (_capi.CassTrack * 1)()
    fresh = ntscsim.FieldSimulator(device=0)
    try:
        assert lib.ntscsim_cass_tracks_device(fresh._h, one, 1, None) == _capi.E_ARG            # no bind
        assert lib.ntscsim_cass_debug_tilt_frames(fresh._h, C.byref(C.c_uint64())) == _capi.E_ARG
    finally:
        fresh.close()
    chain = ntscsim.Cassette(cp, sim=sim)
    buf = torch.zeros(8192, dtype=torch.int16, device="cuda")
    out = torch.full((8192,), 0x5555, dtype=torch.int16, device="cuda")
    states = (torch.arange(3 * SB, dtype=torch.int32) % 251).to(torch.uint8).cuda()
    keep = states.clone()
    base, obase, sbase = buf.data_ptr(), out.data_ptr(), states.data_ptr()
    assert sbase % 8 == 0
    sim.rng_pos = 5

    def call(t0, t1=None, n=None):
        """tracks given as (src, dst, samples, state[, count])"""
        given = [t for t in (t0, t1) if t is not None]
        arr = (_capi.CassTrack * len(given))()
        descs = (_capi.CassDesc * len(given))()
        for t, tr in enumerate(given):
            descs[t].src, descs[t].dst, descs[t].samples, descs[t].rng_pos = tr[0], tr[1], tr[2], _capi.RNG_AUTO
            arr[t].blocks = C.cast(C.byref(descs[t]), C.POINTER(_capi.CassDesc))
            arr[t].n_blocks = 1
            arr[t].state = tr[3]
            arr[t].count = tr[4] if len(tr) > 4 else 0
        return lib.ntscsim_cass_tracks_device(sim._h, arr, len(given) if n is None else n, None)

    ok0, ok1 = (base, obase, 100, sbase), (base + 4096, obase + 4096, 100, sbase + SB)
    assert lib.ntscsim_cass_tracks_device(None, one, 1, None) == _capi.E_ARG                    # a NULL ctx
    assert call(ok0, ok1, n=-1) == _capi.E_ARG
    assert lib.ntscsim_cass_tracks_device(sim._h, None, 1, None) == _capi.E_ARG                 # NULL tracks
    nb = (_capi.CassTrack * 1)()
    nb[0].n_blocks = 1
    assert lib.ntscsim_cass_tracks_device(sim._h, nb, 1, None) == _capi.E_ARG                   # NULL blocks
    assert call(ok0, (None, obase + 4096, 100, None)) == _capi.E_ARG                            # NULL and odd pointers
    assert call(ok0, (base + 4096, None, 100, None)) == _capi.E_ARG
    assert call(ok0, (base + 4097, obase + 4096, 100, None)) == _capi.E_ARG
    assert call(ok0, (base + 4096, obase + 4097, 100, None)) == _capi.E_ARG
    assert call(ok0, (base + 4096, obase + 4096, 100, sbase + SB + 4)) == _capi.E_ARG           # a state not 8-byte aligned
    assert call(ok0, (base + 4096, obase + 4096, 100, sbase)) == _capi.E_ARG                    # two tracks, one state
    assert call(ok0, (base + 4096, obase + 4096, 100, sbase + SB - 8)) == _capi.E_ARG           # overlapping states
    assert call((base, base, 100, sbase)) == _capi.E_ARG                                        # in place
    assert call((base, base + 396, 100, sbase)) == _capi.E_ARG                                  # dst overlaps the end of its src
    assert call(ok0, (base + 4096, base + 396, 100, None)) == _capi.E_ARG                       # dst overlaps the src of another track
    assert call((base + 4096, base + 396, 100, None), ok0) == _capi.E_ARG
    assert call(ok0, ok1 + ((1 << 64) - 100,)) == _capi.E_ARG                                   # count + frames = 2^64
    assert call(ok0, ok1 + ((1 << 64) - 50,)) == _capi.E_ARG
    sim.sync()
    assert sim.rng_pos == 5                                                                     # a refused call draws nothing
    assert bool((out == 0x5555).all()) and not bool(buf.any()) and torch.equal(states, keep)    # and writes nothing
    assert lib.ntscsim_cass_debug_track_stats(sim._h, None, 1) == _capi.E_ARG
    assert lib.ntscsim_cass_debug_tilt_frames(sim._h, None) == _capi.E_ARG
    assert call(ok0, (None, None, 0, None)) == _capi.OK                                         # an empty block needs no pointers
    assert lib.ntscsim_cass_tracks_device(sim._h, None, 0, None) == _capi.OK                    # no tracks at all
    assert sim.rng_pos == 5 + 200
    assert call(ok0, ok1 + ((1 << 64) - 101,)) == _capi.OK                                      # the last count that exists
    sim.sync()
    assert sim.rng_pos == 5 + 200 + 400
    s = (_capi.CassStats * 3)()
    assert lib.ntscsim_cass_debug_track_stats(sim._h, s, 3) == _capi.E_ARG                      # the last call had two tracks
    assert lib.ntscsim_cass_debug_track_stats(sim._h, s, 2) == _capi.OK
    assert (s[0].segments, s[1].segments) == (1, 1)
    assert chain.track_state(states, 1)[1] == (1 << 64) - 1
    assert torch.equal(states[2 * SB:], keep[2 * SB:])                                          # the third state: no track's


def test_the_veneer(sim):
    """process_tracks on tensors of unequal length that are not neighbours, with blocks and positions; states=None"""
    import torch
    cp = T.params(["-deemphasis", "1"])
    frames, counts = [700, 0, 129, 2000], [3, 0, 500, 44100]
    tracks = T.cut(T.make_tracks(frames, seed=90), frames)
    chain = ntscsim.Cassette(cp, sim=sim)
    chain.set_plan(128, 40, 24)
    srcs = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in tracks]
    dsts = [torch.full_like(s, 0x5555) for s in srcs]
    blocks = [[(200, None), (0, None), (500, 9000)], None, [(129, 12)], [(1, None), (1999, None)]]
    want = []
    for t in (0, 2, 3):
        spec = "blocks=" + ",".join("%d:%s" % (n, "a" if p is None else p) for n, p in (blocks[t] or [(frames[t], None)]))
        w, st, pos = A.run_checker(cp, tracks[t], count0=counts[t], rng_pos=2 if t == 0 else pos, block=spec)
        want.append((w, st))
    states = chain.zero_states(4)
    assert states.dtype == torch.uint8 and states.numel() == 4 * 8416 == 4 * chain.STATE_BYTES
    sim.rng_pos = 2
    chain.process_tracks(srcs, dsts, counts, states, blocks)
    chain.sync()
    assert sim.rng_pos == pos
    for (w, st), t in zip(want, (0, 2, 3)):
        assert (dsts[t].cpu().numpy() == w).all(), t
        vals, count, hist = chain.track_state(states, t)
        assert count == st[1] and (np.array(vals).view(np.uint64) == st[0]).all() and (np.array(hist).view(np.uint64) == st[2]).all()
    assert [s[0] for s in chain.track_stats(4)] == [6, 0, 2, 16]
    assert chain.track_state(states, 1) == (tuple([0.0] * 28), 0, tuple([(0.0, 0.0)] * 7))     # a track without frames leaves its state
    dsts2 = [torch.full_like(s, 0x5555) for s in srcs]
    sim.rng_pos = 2
    chain.process_tracks(srcs, dsts2, counts, None, blocks)
    chain.sync()
    for (w, _), t in zip(want, (0, 2, 3)):
        assert (dsts2[t].cpu().numpy() == w).all(), t
    chain.set_plan(0, 0, 0)
