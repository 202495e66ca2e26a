"""Cassette tracks with parameters per track in one call (ntscsim_cass_mixed_tracks_device / _host: k_audio_hiss,
k_cass_mixed_front, k_cass_mixed_front_verify, k_cass_mixed_conv, k_cass_mixed_back, k_cass_mixed_back_verify) against
the serial chain of csrc/cass_chain.hpp run PER TRACK with that track's own parameters, state and count, every tap of
the FIR and this host's sines (tests/cass_mixed_tracks_check.cpp `expect`, one process per track set;
tests/test_cass_mixed_tracks_host.py pins that mode to tests/cass_tracks_check.cpp's).  The chain is exact arithmetic,
so the tolerance is zero: output bytes, the whole state byte for byte -- the 28 filter values, the count, the taps, the
track's own taps - 1 history frames and the rest of the history, which must stay as it came -- and the ctx's rand()
position.  The expectation is never the code under test, but where a test says that two forms of the call are equal.

Shapes are tests/_cass_tracks.py's, the smallest at which the indexing can go wrong; the tracks are cut back to back
from one device buffer with different content in each, the destination is pre-filled with a pattern and the source is
compared afterwards."""
import ctypes as C

import numpy as np
import pytest

import _cass_mixed as M
import _cass_ref as A
import _cass_tracks as T
import ntscsim
from ntscsim import _capi

pytestmark = pytest.mark.gpu
SB = T.STATE_BYTES
FRONT = ["k_cass_mixed_front", "k_cass_mixed_front_verify", "k_cass_mixed_conv"]
BACK = ["k_cass_mixed_back", "k_cass_mixed_back_verify"]


@pytest.fixture(scope="module")
def sim():
    s = ntscsim.FieldSimulator(device=0)
    yield s
    s.close()


def state_tensor(raw):
    import torch
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()


def mixed_args(sets, set_of, src_ptr, dst_ptr, frames, counts, state_ptrs):
    """The C arrays of a mixed call over tracks cut back to back from one source and one destination."""
    n = len(frames)
    arr = (_capi.CassParams * max(1, len(sets)))(*sets)
    tracks = (_capi.CassMixedTrack * max(1, n))()
    descs = (_capi.CassDesc * max(1, n))()
    at = 0
    for t, f in enumerate(frames):
        descs[t].src, descs[t].dst = src_ptr + at * 4, dst_ptr + at * 4
        descs[t].samples, descs[t].rng_pos = f, _capi.RNG_AUTO
        tracks[t].blocks = C.cast(C.byref(descs[t]), C.POINTER(_capi.CassDesc))
        tracks[t].n_blocks = 1
        tracks[t].set = set_of[t]
        tracks[t].count = counts[t]
        tracks[t].state = state_ptrs[t]
        at += f
    return arr, tracks, descs


def launch(sim, chain, sets, set_of, src, dst, frames, counts, states, slots=None, stream=None, want_rc=_capi.OK):
    """One mixed call over tracks cut back to back from src / dst.  slots: None (track t on state t of `states`, through
    the veneer) or per track a state index or None for a NULL state (through the C ABI).  Does not synchronise."""
    if slots is None:
        chain.process_mixed_tracks(sets, set_of, T.cut(src, frames), T.cut(dst, frames), counts, states, stream=stream)
        return
    ptrs = [None if s is None else states.data_ptr() + s * SB for s in slots]
    arr, tracks, _descs = mixed_args(sets, set_of, src.data_ptr(), dst.data_ptr(), frames, counts, ptrs)
    rc = sim._lib.ntscsim_cass_mixed_tracks_device(sim._h, arr if sets else None, len(sets), tracks, len(frames),
                                                   C.c_void_p(stream if stream is not None else sim._torch_stream()))
    assert rc == want_rc


def run_mixed(sim, chain, sets, set_of, whole, frames, counts, states, slots=None):
    import torch
    src = torch.from_numpy(np.ascontiguousarray(whole)).cuda()
    dst = torch.full_like(src, 0x5555)
    launch(sim, chain, sets, set_of, src, dst, frames, counts, states, slots)
    chain.sync()
    assert torch.equal(src.cpu(), torch.from_numpy(np.ascontiguousarray(whole))), "the call wrote its source"
    return T.cut(dst.cpu().numpy(), frames)


def assert_tracks(got, want, states=None, want_states=None, skip=(), what=""):
    for t, (g, w) in enumerate(zip(got, want)):
        bad = int((g != w).sum())
        first = int(np.argmax((g != w).reshape(-1))) if bad else -1
        assert bad == 0, "%s track %d: %d wrong samples, first at %d" % (what, t, bad, first)
    if states is not None:
        raw = states if isinstance(states, bytes) else states.cpu().numpy().tobytes()
        for t in range(len(raw) // SB):
            if t in skip:
                continue
            a, b = raw[t * SB:(t + 1) * SB], want_states[t * SB:(t + 1) * SB]
            if a != b:
                x, y = _capi.CassState.from_buffer_copy(a), _capi.CassState.from_buffer_copy(b)
                diff = [i for i in range(0, SB, 8) if a[i:i + 8] != b[i:i + 8]]
                raise AssertionError("%s state %d: count %d / %d, taps %d / %d, first differing doubles at bytes %s" % (what, t, x.count, y.count, x.taps, y.taps, diff[:6]))


def lead_in(sets, set_of, counts, seed=77, frames=100):
    """States with a non-zero history of every track's own length: what the serial chain leaves behind a lead-in that
    ends at counts[t]."""
    n = len(set_of)
    lead = T.make_tracks([frames] * n, seed=seed)
    _, states, _ = M.expect(sets, set_of, lead, [frames] * n, [c - frames for c in counts])
    for t in range(n):
        s = _capi.CassState.from_buffer_copy(states[t * SB:(t + 1) * SB])
        assert s.taps == sets[set_of[t]].taps and s.count == counts[t] and any(s.history[k][0] != 0.0 for k in range(s.taps - 1))
    return states


def test_six_decks_in_one_wavefront(sim):
    """8 and 57 taps, pre-emphasis on and off, two hiss levels and none, -high 100 next to 20 Hz, mono, de-emphasis on
    some only; the 1- and 2-frame tracks sit on 57-tap decks with a carried history"""
    sets = M.decks()
    chain = ntscsim.Cassette(sets[5], sim=sim)
    for plan, frames in T.STRADDLE_PLANS:
        n = len(frames)
        set_of, counts = M.cycle(n), [100] * n
        assert all(sets[set_of[t]].taps == 57 for t in (1, 6) if t < n)
        start = lead_in(sets, set_of, counts)
        a = T.make_tracks(frames)
        want, wst, pos = M.expect(sets, set_of, a, frames, counts, states_in=start, rng_pos=3)
        chain.set_plan(*plan)
        sim.rng_pos = 3
        states = state_tensor(start)
        got = run_mixed(sim, chain, sets, set_of, a, frames, counts, states)
        assert_tracks(got, want, states, wst, what="plan %s" % (plan,))
        assert sim.rng_pos == pos
        stats = chain.track_stats(n)
        assert [s[0] for s in stats] == [(f + plan[0] - 1) // plan[0] for f in frames], plan
        assert all(s[2] == 0 for s, k in zip(stats, set_of) if not sets[k].deemphasis)
        assert chain.tilt_frames() == max(frames)
        assert sim.last_kernels() == ["k_audio_hiss"] + FRONT + BACK
        # from zero states the repairs are the host plan's
        host_stats, hpos, htilt = M.run_check(sets, set_of, a, frames, [0] * n, plan, rng_pos=3)
        sim.rng_pos = 3
        run_mixed(sim, chain, sets, set_of, a, frames, [0] * n, chain.zero_states(n))
        assert chain.track_stats(n) == host_stats and sim.rng_pos == hpos and chain.tilt_frames() == htilt
    chain.set_plan(0, 0, 0)


@pytest.mark.parametrize("post", [False, True], ids=["plain", "deemphasis"])
def test_tiles_with_alternating_taps(sim, post):
    """The tile edges, a one-frame last tile, three tiles in one track, a track without frames; 8 and 57 taps alternate,
    so the halo of a 57-tap track's first tile stands behind an 8-tap track's section.  Every track starts from a
    non-zero history."""
    extra = ["-deemphasis", "1"] if post else []
    sets = [T.params(extra), T.params(A.BAD_DECK + extra)]
    n = len(T.TILES)
    set_of, counts = [0, 1, 0, 1, 0], [100, 1100, 105, 177, 100100]
    start = lead_in(sets, set_of, counts)
    a = T.make_tracks(T.TILES)
    want, wst, pos = M.expect(sets, set_of, a, T.TILES, counts, states_in=start, rng_pos=9)
    chain = ntscsim.Cassette(sets[0], sim=sim)
    sim.rng_pos = 9
    states = state_tensor(start)
    got = run_mixed(sim, chain, sets, set_of, a, T.TILES, counts, states)
    assert_tracks(got, want, states, wst)
    assert sim.rng_pos == pos
    assert wst[3 * SB:4 * SB] == start[3 * SB:4 * SB]                           # the track without frames: as it came
    assert [s[0] for s in chain.track_stats(n)] == [1, 1, 1, 0, 1]
    assert sim.last_kernels() == ["k_audio_hiss"] + FRONT + (BACK if post else [])


def test_sines_are_shared_across_tilt_and_waver(sim):
    tilts = [T.params(["-headalign", str(h), "-headalignwaver", str(w)]) for h, w in ((0, 0), (1, 2), (-3, 1), (10, 3))]
    frames, counts = [300, 200, 250, 100], [0] * 4
    a = T.make_tracks(frames)
    chain = ntscsim.Cassette(tilts[0], sim=sim)
    want, wst, pos = M.expect(tilts, [0, 1, 2, 3], a, frames, counts, rng_pos=1)
    sim.rng_pos = 1
    states = chain.zero_states(4)
    got = run_mixed(sim, chain, tilts, [0, 1, 2, 3], a, frames, counts, states)
    assert_tracks(got, want, states, wst, what="four tilts")
    assert sim.rng_pos == pos and chain.tilt_frames() == max(frames)
    # a set on another rate at the same counts has sines of its own
    sets = tilts + [M.params(["-headalign", "1"], rate=48000)]
    frames, counts = frames + [150], counts + [0]
    a = T.make_tracks(frames)
    want, wst, pos = M.expect(sets, [0, 1, 2, 3, 4], a, frames, counts, rng_pos=1)
    sim.rng_pos = 1
    states = chain.zero_states(5)
    got = run_mixed(sim, chain, sets, [0, 1, 2, 3, 4], a, frames, counts, states)
    assert_tracks(got, want, states, wst, what="two rates")
    assert sim.rng_pos == pos and chain.tilt_frames() == 300 + 150


def test_rand_positions(sim):
    """Hissing and silent tracks interleaved; NTSCSIM_RNG_AUTO and explicit positions, some backward.  A block moves the
    position by 2 * samples only when its track draws; an explicit position is taken from any block."""
    import torch
    sets = [T.params([]), T.params(["-audio-hiss", "-200"]), T.params(A.BAD_DECK)]
    set_of, frames, counts = [0, 1, 2, 1, 0], [300, 200, 150, 0, 260], [0, 7, 0, 0, 1 << 33]
    blocks = [[(100, None), (200, 5000)], [(50, 40), (150, None)], [(150, None)], [(0, 9)], [(60, 2), (0, 777), (200, None)]]
    tracks = T.cut(T.make_tracks(frames, seed=31), frames)
    pos, want = 11, []
    for t, (a, cut) in enumerate(zip(tracks, blocks)):
        cp = sets[set_of[t]]
        if len(a):
            spec = "blocks=" + ",".join("%d:%s" % (n, "a" if p is None else p) for n, p in cut)
            w, _st, p2 = A.run_checker(cp, a, count0=counts[t], rng_pos=pos, block=spec)
            want.append(w)
        else:
            want.append(a)
        for n, p in cut:                                                        # the rule, stated here
            pos = pos if p is None else p
            pos += 2 * n if cp.hiss_level else 0
        assert not (len(a) and cp.hiss_level) or p2 == pos
    assert pos == 777 + 400
    chain = ntscsim.Cassette(sets[0], sim=sim)
    srcs = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in tracks]
    dsts = [torch.full_like(s, 0x5555) for s in srcs]
    sim.rng_pos = 11
    chain.process_mixed_tracks(sets, set_of, srcs, dsts, counts, None, blocks)
    assert sim.rng_pos == pos                                                   # at call time
    chain.sync()
    assert_tracks([d.cpu().numpy() for d in dsts], want)


def test_repairs_in_one_track_only(sim):
    sets = [T.params(T.NO_HISS_DEEMPH), T.params(["-audio-hiss", "-200"])]
    frames, counts, set_of = [3000, 3000, 3000], [0, 0, 0], [0, 0, 1]
    a = T.make_tracks(frames, ["music", "silence", "music"])
    want, wst, _ = M.expect(sets, set_of, a, frames, counts)
    host_stats, _, _ = M.run_check(sets, set_of, a, frames, counts, (256, 0, 0))
    chain = ntscsim.Cassette(sets[1], sim=sim)
    chain.set_plan(256, 0, 0)
    states = chain.zero_states(3)
    got = run_mixed(sim, chain, sets, set_of, a, frames, counts, states)
    assert_tracks(got, want, states, wst)
    assert not got[1].any()
    stats = chain.track_stats(3)
    assert stats == host_stats and stats[1] == (12, 0, 0) and stats[0][1] == 11 and stats[0][2] > 0 and stats[2] == (12, 11, 0)
    chain.set_plan(0, 0, 0)


def test_default_plan_warms_up_per_track(sim):
    """Three tracks of 60000 frames at 20 Hz interleaved with three of 12000 at -high 100, the SHORT warm-up's set
    bound: a call-wide warm-up of 5056 frames would leave the 20 Hz tracks to be repaired."""
    sets = [T.params([]), T.params(["-high", "100"])]
    frames, set_of, counts = [60000, 12000] * 3, [0, -1] * 3, [0] * 6
    a = T.make_tracks(frames)
    want, wst, pos = M.expect(sets, [0, 1] * 3, a, frames, counts, rng_pos=1000)
    host_stats, _, _ = M.run_check(sets, [0, 1] * 3, a, frames, counts, (4096, -1, -1), rng_pos=1000)
    chain = ntscsim.Cassette(sets[1], sim=sim)
    assert chain.default_warmups()[0] == 5056
    sim.rng_pos = 1000
    states = chain.zero_states(6)
    got = run_mixed(sim, chain, sets[:1], set_of, a, frames, counts, states)
    assert_tracks(got, want, states, wst)
    assert sim.rng_pos == pos
    assert chain.track_stats(6) == host_stats == [((f + 4095) // 4096, 0, 0) for f in frames]
    assert chain.tilt_frames() == 60000 and sim.last_kernels() == ["k_audio_hiss"] + FRONT


def test_special_forms(sim):
    import torch
    cp = T.params(A.BAD_DECK + T.BOTH)
    other = T.params([])
    frames, counts = [700, 0, 129, 2000], [3, 0, 500, 3000000000 * 3600]       # the last: hours into a tape
    a = T.make_tracks(frames, seed=90)
    chain = ntscsim.Cassette(cp, sim=sim)
    chain.set_plan(128, 40, 24)
    # one set == the tracks call, byte for byte
    src = torch.from_numpy(a).cuda()
    d1, d2, d3, d4 = (torch.full_like(src, 0x5555) for _ in range(4))
    s1, s2, s3, s4 = (chain.zero_states(4) for _ in range(4))
    sim.rng_pos = 2
    chain.process_tracks(T.cut(src, frames), T.cut(d1, frames), counts, s1)
    chain.sync()
    pos1, stats1, tilt1 = sim.rng_pos, chain.track_stats(4), chain.tilt_frames()
    sim.rng_pos = 2
    launch(sim, chain, [other, cp], [1] * 4, src, d2, frames, counts, s2)
    chain.sync()
    assert torch.equal(d1, d2) and torch.equal(s1, s2) and sim.rng_pos == pos1
    assert chain.track_stats(4) == stats1 and chain.tilt_frames() == tilt1
    # set == -1 with n_sets == 0: the bound parameters
    sim.rng_pos = 2
    launch(sim, chain, [], [-1] * 4, src, d3, frames, counts, s3, slots=[0, 1, 2, 3])
    chain.sync()
    assert torch.equal(d1, d3) and torch.equal(s1, s3) and sim.rng_pos == pos1
    # a NULL state; garbage count and taps on entry
    raw = bytearray(4 * SB)
    for t in range(4):
        s = _capi.CassState.from_buffer(raw, t * SB)
        s.count, s.taps = 0xDEADBEEF00 + t, 4000 + t
    want, wst, pos = M.expect([other, cp], [1, 0, 0, 1], a, frames, counts, states_in=bytes(raw), null=(2,), rng_pos=2)
    s4 = state_tensor(raw)
    sim.rng_pos = 2
    launch(sim, chain, [other, cp], [1, 0, 0, 1], src, d4, frames, counts, s4, slots=[0, 1, None, 3])
    chain.sync()
    assert_tracks(T.cut(d4.cpu().numpy(), frames), want, s4, wst, what="garbage on entry")
    assert sim.rng_pos == pos
    assert chain.track_state(s4, 3)[1] == counts[3] + 2000
    # two calls in sequence on the same states == one call over both
    first = [f // 3 for f in frames]
    rest = [f - p for f, p in zip(frames, first)]
    a1 = np.concatenate([x[:p] for x, p in zip(T.cut(a, frames), first)])
    a2 = np.concatenate([x[p:] for x, p in zip(T.cut(a, frames), first)])
    states = chain.zero_states(4)
    sim.rng_pos = 2
    g1 = run_mixed(sim, chain, [other, cp], [1, 0, 0, 1], a1, first, counts, states)
    mid = sim.rng_pos
    g2 = run_mixed(sim, chain, [other, cp], [1, 0, 0, 1], a2, rest, [c + p for c, p in zip(counts, first)], states)
    # the draws of a split run interleave differently: compare with the expectation of the same two calls
    w1, st1, p1 = M.expect([other, cp], [1, 0, 0, 1], a1, first, counts, rng_pos=2)
    w2, st2, p2 = M.expect([other, cp], [1, 0, 0, 1], a2, rest, [c + p for c, p in zip(counts, first)], states_in=st1, rng_pos=p1)
    assert_tracks(g1, w1, what="first call")
    assert_tracks(g2, w2, states, st2, what="second call")
    assert mid == p1 and sim.rng_pos == p2
    # ... and where no track draws, the two calls are the one call
    quiet = [T.params(["-audio-hiss", "-200"]), T.params(A.BAD_DECK + T.NO_HISS_DEEMPH)]
    want, wst, _ = M.expect(quiet, [1, 0, 0, 1], a, frames, counts)
    states = chain.zero_states(4)
    g1 = run_mixed(sim, chain, quiet, [1, 0, 0, 1], a1, first, counts, states)
    g2 = run_mixed(sim, chain, quiet, [1, 0, 0, 1], a2, rest, [c + p for c, p in zip(counts, first)], states)
    assert_tracks([np.concatenate([x, y]) for x, y in zip(g1, g2)], want, states, wst, skip=(1,), what="two calls, one stream")
    chain.set_plan(0, 0, 0)


def test_many_tracks_and_many_sets(sim):
    """1,100 tracks of 8 frames over 7 sets; 300 sets on 300 tracks"""
    seven = M.decks() + [T.params(["-preset", "0"])]
    assert seven[6].taps == 25
    set_of = [t % 7 for t in range(T.MANY)]
    frames, counts = [8] * T.MANY, [1000 * t for t in range(T.MANY)]
    a = T.make_tracks(frames, seed=5)
    want, wst, pos = M.expect(seven, set_of, a, frames, counts, rng_pos=4)
    chain = ntscsim.Cassette(seven[0], sim=sim)
    sim.rng_pos = 4
    states = chain.zero_states(T.MANY)
    got = run_mixed(sim, chain, seven, set_of, a, frames, counts, states)
    assert_tracks(got, want, states, wst, what="1100 tracks")
    assert sim.rng_pos == pos and chain.tilt_frames() == 8 * T.MANY
    many = []
    for i in range(300):
        cp = T.params(["-headalign", str(i % 21 - 10), "-audio-hiss", str(-30 - i % 40)] + (["-deemphasis", "1"] if i % 3 == 0 else []))
        many.append(cp)
    frames, counts = [40] * 300, [0] * 300
    a = T.make_tracks(frames, seed=6)
    want, wst, pos = M.expect(many, list(range(300)), a, frames, counts, rng_pos=4)
    sim.rng_pos = 4
    states = chain.zero_states(300)
    got = run_mixed(sim, chain, many, list(range(300)), a, frames, counts, states)
    assert_tracks(got, want, states, wst, what="300 sets")
    assert sim.rng_pos == pos and chain.tilt_frames() == 40


def test_in_flight_behind_other_calls_and_the_ctx_is_left_alone():
    """On one stream that is not the default one, without a wait: a tracks call, a mixed call, a plain call.  The plain
    call starts from the ctx's own state and runs on the bound parameters, as if no mixed call had been."""
    import torch
    cp = T.params(A.BAD_DECK + ["-deemphasis", "1"])
    sets = M.decks()
    frames, counts = [600, 1, 0, 193, 900], [0, 10, 20, 3000000000, 40]
    set_of = M.cycle(5)
    a = T.make_tracks(frames, seed=60)
    ap = A.make_input("music", 700, 2, 33)
    want1, st1, pos1 = T.expect(cp, a, frames, counts, rng_pos=2)
    want2, st2, pos2 = M.expect(sets, set_of, a, frames, counts, rng_pos=pos1)
    wantp, stp, posp = A.run_checker(cp, ap, rng_pos=pos2)
    sim = ntscsim.FieldSimulator(device=0)
    try:
        chain = ntscsim.Cassette(cp, sim=sim)
        src, srcp = torch.from_numpy(np.ascontiguousarray(a)).cuda(), torch.from_numpy(ap).cuda()
        o1, o2, op = torch.full_like(src, 0x5555), torch.full_like(src, 0x5555), torch.full_like(srcp, 0x5555)
        s1, s2 = chain.zero_states(5), chain.zero_states(5)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        sim.rng_pos = 2
        chain.process_tracks(T.cut(src, frames), T.cut(o1, frames), counts, s1, stream=stream.cuda_stream)
        launch(sim, chain, sets, set_of, src, o2, frames, counts, s2, stream=stream.cuda_stream)
        chain.process(srcp, op, stream=stream.cuda_stream)
        assert sim.rng_pos == posp
        stream.synchronize()
        chain.sync()
        assert_tracks(T.cut(o1.cpu().numpy(), frames), want1, s1, st1, what="tracks call")
        assert_tracks(T.cut(o2.cpu().numpy(), frames), want2, s2, st2, what="mixed call")
        assert (op.cpu().numpy() == wantp).all()
        vals, count, hist = chain.state
        assert count == stp[1] == 700 and (np.array(vals).view(np.uint64) == stp[0]).all()
        assert (np.array(hist).view(np.uint64).reshape(-1, 2) == stp[2]).all()
    finally:
        sim.close()


def test_refusals(sim):
    """Every refusal leaves the rand() position, the states and the destination as they were; the next call is exact."""
    import torch
    lib = sim._lib
    good, other = T.params([]), T.params(A.BAD_DECK)
    fresh = ntscsim.FieldSimulator(device=0)
    try:
        one = (_capi.CassMixedTrack * 1)()
        one[0].set = -1
        assert lib.ntscsim_cass_mixed_tracks_device(fresh._h, None, 0, one, 1, None) == _capi.E_ARG    # no bind
        assert lib.ntscsim_cass_mixed_tracks_host(fresh._h, None, 0, one, 1) == _capi.E_ARG
    finally:
        fresh.close()
    chain = ntscsim.Cassette(good, sim=sim)
    buf = torch.zeros(8192, dtype=torch.int16, device="cuda")
    out = torch.full((8192,), 0x5555, dtype=torch.int16, device="cuda")
    states = (torch.arange(3 * SB, dtype=torch.int32) % 251).to(torch.uint8).cuda()
    keep = states.clone()
    base, obase, sbase = buf.data_ptr(), out.data_ptr(), states.data_ptr()
    sim.rng_pos = 5

    def call(t0, t1=None, n=None, sets=(good, other), n_sets=None, null_sets=False):
        """tracks given as (src, dst, samples, state, set[, count])"""
        given = [t for t in (t0, t1) if t is not None]
        arr = (_capi.CassParams * max(1, len(sets)))(*sets)
        tracks = (_capi.CassMixedTrack * len(given))()
        descs = (_capi.CassDesc * len(given))()
        for t, tr in enumerate(given):
            descs[t].src, descs[t].dst, descs[t].samples, descs[t].rng_pos = tr[0], tr[1], tr[2], _capi.RNG_AUTO
            tracks[t].blocks = C.cast(C.byref(descs[t]), C.POINTER(_capi.CassDesc))
            tracks[t].n_blocks = 1
            tracks[t].state = tr[3]
            tracks[t].set = tr[4]
            tracks[t].count = tr[5] if len(tr) > 5 else 0
        return lib.ntscsim_cass_mixed_tracks_device(sim._h, None if null_sets else arr, len(sets) if n_sets is None else n_sets, tracks,
                                                    len(given) if n is None else n, None)

    ok0, ok1 = (base, obase, 100, sbase, 0), (base + 4096, obase + 4096, 100, sbase + SB, 1)
    E = _capi.E_ARG
    assert lib.ntscsim_cass_mixed_tracks_device(None, None, 0, None, 0, None) == E                # a NULL ctx
    assert call(ok0, ok1, n=-1) == E
    assert lib.ntscsim_cass_mixed_tracks_device(sim._h, None, 0, None, 1, None) == E              # NULL tracks
    nb = (_capi.CassMixedTrack * 1)()
    nb[0].n_blocks, nb[0].set = 1, -1
    assert lib.ntscsim_cass_mixed_tracks_device(sim._h, None, 0, nb, 1, None) == E                # NULL blocks
    assert call(ok0, (None, obase + 4096, 100, None, 1)) == E                                     # NULL and odd pointers
    assert call(ok0, (base + 4096, None, 100, None, 1)) == E
    assert call(ok0, (base + 4097, obase + 4096, 100, None, 1)) == E
    assert call(ok0, (base + 4096, obase + 4097, 100, None, 1)) == E
    assert call(ok0, (base + 4096, obase + 4096, 100, sbase + SB + 4, 1)) == E                    # a state not 8-byte aligned
    assert call(ok0, (base + 4096, obase + 4096, 100, sbase, 1)) == E                             # two tracks, one state
    assert call(ok0, (base + 4096, obase + 4096, 100, sbase + SB - 8, 1)) == E                    # overlapping states
    assert call((base, base, 100, sbase, 0)) == E                                                 # in place
    assert call(ok0, (base + 4096, base + 396, 100, None, 1)) == E                                # dst overlaps another track's src
    assert call(ok0, ok1 + ((1 << 64) - 100,)) == E                                               # count + frames = 2^64
    assert call(ok0, ok1[:4] + (2,)) == E                                                         # a set outside -1 .. n_sets-1
    assert call(ok0, ok1[:4] + (-2,)) == E
    assert call(ok0, ok1, n_sets=-1) == E
    assert call(ok0, ok1, null_sets=True) == E                                                    # NULL sets that should hold something
    wrong = T.params([])
    wrong.struct_size -= 8
    assert call(ok0, ok1, sets=(good, wrong)) == E                                                # a named set with a wrong struct_size
    sim.sync()
    assert sim.rng_pos == 5                                                                       # a refused call draws nothing
    assert bool((out == 0x5555).all()) and not bool(buf.any()) and torch.equal(states, keep)      # and writes nothing
    for field, value in (("taps", 9), ("channels", 1), ("passes", 5), ("rate", 0), ("hiss_level", -1), ("highpass_hz", 0.0)):
        badp = T.params([])
        setattr(badp, field, value)
        assert call(ok0, ok1, sets=(good, badp)) == _capi.E_PARAM, field                          # what ntscsim_cass_bind() refuses
        assert call(ok0, ok1[:4] + (0,), sets=(good, badp)) == _capi.OK                           # a set no track names is not looked at
        sim.sync()
        assert sim.rng_pos == 5 + 400
        sim.rng_pos = 5
        states.copy_(keep)
        out.fill_(0x5555)
    sim.sync()
    assert sim.rng_pos == 5                                                                       # a refused call draws nothing
    assert bool((out == 0x5555).all()) and not bool(buf.any()) and torch.equal(states, keep)      # and writes nothing
    assert sim.last_kernels()[-1] == "k_cass_mixed_conv"                                          # the last accepted call's
    assert call(ok0, (None, None, 0, None, 1)) == _capi.OK                                        # an empty block needs no pointers
    assert lib.ntscsim_cass_mixed_tracks_device(sim._h, None, 0, None, 0, None) == _capi.OK       # no tracks at all
    assert sim.rng_pos == 5 + 200
    # the next call is exact
    a = T.make_tracks([100, 100], seed=3)
    want, wst, pos = M.expect([good, other], [0, 1], a, [100, 100], [0, 0], rng_pos=5)
    sim.rng_pos = 5
    st = chain.zero_states(2)
    got = run_mixed(sim, chain, [good, other], [0, 1], a, [100, 100], [0, 0], st)
    assert_tracks(got, want, st, wst, what="behind the refusals")
    assert sim.rng_pos == pos


def test_the_host_form(sim):
    """In place, on odd addresses, with host states; two tracks on one state are refused."""
    sets = M.decks()
    frames, counts = [300, 1, 0, 193, 257], [100, 110, 120, 3000000000, 140]
    set_of = M.cycle(5)
    a = T.make_tracks(frames, seed=61)
    start = lead_in(sets, set_of, counts)
    want, wst, pos = M.expect(sets, set_of, a, frames, counts, states_in=start, rng_pos=8)
    chain = ntscsim.Cassette(sets[3], sim=sim)
    chain.set_plan(64, 20, 16)
    raw = np.zeros(sum(frames) * 4 + 2 * len(frames) + 1, np.uint8)
    arrays, at = [], 1                                                          # every track starts on an odd address
    for x in T.cut(a, frames):
        v = raw[at:at + x.size * 2].view(np.int16).reshape(-1, 2)
        assert v.ctypes.data % 2 == 1 or x.size == 0
        v[...] = x
        arrays.append(v)
        at += x.size * 2 + 2
    sraw = np.zeros(5 * SB + 1, np.uint8)
    st = sraw[1:]                                                               # host states on an odd address
    st[:] = np.frombuffer(start, np.uint8)
    sim.rng_pos = 8
    chain.host_mixed_tracks(sets, set_of, arrays, counts, st)
    assert sim.rng_pos == pos
    assert_tracks(arrays, want, st.tobytes(), wst, what="host form")
    assert [s[0] for s in chain.track_stats(5)] == [(f + 63) // 64 for f in frames]
    # two tracks on one state
    arr, tracks, _d = mixed_args(sets, set_of[:2], raw.ctypes.data, raw.ctypes.data, [10, 10], [0, 0], [st.ctypes.data, st.ctypes.data])
    keep = raw.copy()
    assert sim._lib.ntscsim_cass_mixed_tracks_host(sim._h, arr, len(sets), tracks, 2) == _capi.E_ARG
    assert sim.rng_pos == pos and (raw == keep).all()
    chain.set_plan(0, 0, 0)


def test_the_bound_parameters_and_the_ctx_state_stay(sim):
    """a plain call behind a mixed call equals one without the mixed call before it"""
    import torch
    cp = T.params(["-preset", "0", "-preemphasis", "1", "-deemphasis", "1"])     # 25 taps
    a = A.make_input("music", 3000, 2, 8)
    chain = ntscsim.Cassette(cp, sim=sim)
    src = torch.from_numpy(a).cuda()
    outs = []
    for mixed in (False, True):
        chain.state = (tuple([0.25] * 28), 12345, tuple([(0.5, -0.5)] * 24))
        if mixed:
            sets = M.decks()
            frames = [500, 700]
            b = T.make_tracks(frames)
            run_mixed(sim, chain, sets, [1, 2], b, frames, [9, 9], chain.zero_states(2))
        dst = torch.full_like(src, 0x5555)
        sim.rng_pos = 1
        chain.process(src, dst)
        chain.sync()
        outs.append((dst.cpu().numpy(), chain.state, sim.rng_pos, chain.stats()))
    assert (outs[0][0] == outs[1][0]).all() and outs[0][1:] == outs[1][1:]
    assert outs[0][1][1] == 12345 + 3000
