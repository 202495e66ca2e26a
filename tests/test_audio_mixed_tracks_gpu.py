"""Independent audio tracks with parameters PER TRACK in one call (ntscsim_audio_mixed_tracks_device / _host:
k_audio_hiss, k_audio_mixed_pulses, k_audio_mixed_segments, k_audio_mixed_verify) against the host checker run PER TRACK
with that track's parameters (A.run_checker: the serial chain of csrc/audio_chain.hpp, which tests/test_audio_ref.py pins
to the reference's own lines), the rand() position chained through the tracks, byte for byte and state bit for state
bit: the chain is exact arithmetic, so the tolerance is zero.  The expectation is never the code under test, but for
test_equivalences, whose expectation is the existing tracks call.

Shapes are those of tests/test_audio_tracks_gpu.py (the smallest at which the indexing can go wrong), with the tracks
cycling through sets so that the three groups of a wavefront differ in channels, buzz, hiss and enabled.  The tracks
are cut back to back from one device buffer with different content in each."""
import ctypes as C

import numpy as np
import pytest

import _audio_mixed as M
import _audio_ref as A
import _audio_tracks as T
import ntscsim
from ntscsim import _capi

pytestmark = pytest.mark.gpu

KERNELS = ["k_audio_hiss", "k_audio_mixed_pulses", "k_audio_mixed_segments", "k_audio_mixed_verify"]


@pytest.fixture(scope="module")
def sim():
    s = ntscsim.FieldSimulator(device=0)
    yield s
    s.close()


def run_mixed(chain, sets, set_of, tracks, states=None, blocks=None):
    """The tracks back to back in one device buffer, through one mixed call: the outputs as numpy arrays."""
    import torch
    sizes = [a.size for a in tracks]
    whole = np.concatenate([np.ascontiguousarray(a).reshape(-1) for a in tracks] + [np.zeros(0, np.int16)])
    src = torch.from_numpy(whole).cuda()
    dst = torch.full_like(src, 0x5555)
    chain.process_mixed_tracks(sets, set_of, T.cut(src, sizes), T.cut(dst, sizes), states, blocks)
    chain.sync()
    assert torch.equal(src.cpu(), torch.from_numpy(whole)), "the call wrote its source"
    return [np.array(x).reshape(a.shape) for x, a in zip(T.cut(dst.cpu().numpy(), sizes), tracks)]


def assert_tracks(got, want, states=None, before=None, what=""):
    """want[t]: (output, (values, count)); (output, None) for a copied track, whose state must be what `before` held"""
    for t, (g, (w, st)) in enumerate(zip(got, want)):
        bad = int((g != w).sum())
        first = int(np.argmax((g != w).reshape(-1))) if bad else -1
        assert bad == 0, "%s track %d: %d wrong samples, first at %d" % (what, t, bad, first)
        if states is None:
            continue
        vals, count = ntscsim.AudioChain.track_state(states, t)
        if st is None:
            st = before[t] if before is not None else (tuple([0.0] * 30), 0)
        assert count == st[1], "%s track %d" % (what, t)
        assert (A.state_bits(vals) == A.state_bits(st[0])).all(), "%s track %d" % (what, t)


def test_the_feature_exists(sim):
    """One call, two tracks of 4096 frames, stereo Hi-Fi next to mono linear LP."""
    sets, set_of = M.sets_of(["stereo_hifi", "mono_lp"]), [0, 1]
    assert hasattr(sim._lib, "ntscsim_audio_mixed_tracks_device")
    tracks = M.make_tracks([4096, 4096], sets, set_of, seed=21)
    want, pos = M.expect(sets, set_of, tracks)
    sim.rng_pos = 0
    chain = ntscsim.AudioChain(sets[0], sim=sim)
    states = chain.zero_states(2)
    got = run_mixed(chain, sets, set_of, tracks, states)
    assert_tracks(got, want, states)
    assert sim.rng_pos == pos == 3 * 4096


def test_three_sets_in_one_wavefront(sim):
    sets = M.sets_of(M.CYCLE)
    chain = ntscsim.AudioChain(sets[1], sim=sim)
    for plan, frames in (((64, 20), T.STRADDLE), ((1, 0), T.STRADDLE[:4]), ((65, 64), T.STRADDLE[:4])):
        set_of = [t % len(sets) for t in range(len(frames))]
        tracks = M.make_tracks(frames, sets, set_of)
        want, pos = M.expect(sets, set_of, tracks, pos=3)
        chain.set_plan(*plan)
        sim.rng_pos = 3
        states = chain.zero_states(len(frames))
        got = run_mixed(chain, sets, set_of, tracks, states)
        assert_tracks(got, want, states, what="plan %s" % (plan,))
        assert sim.rng_pos == pos
        stats = chain.track_stats(len(frames))
        assert [s[0] for s in stats] == [(f + plan[0] - 1) // plan[0] if sets[s].enabled else 0 for f, s in zip(frames, set_of)], plan
        if plan == (64, 20):
            assert sim.last_kernels() == KERNELS                                 # one launch of each, however many sets
    chain.set_plan(0, 0)


def test_per_track_default_warmup(sim):
    """Zero repairs is a condition on these inputs, shown on the CPU by tests/test_audio_mixed_tracks_host.py
    (test_default_plan_sets_need_no_repair runs the same generator inputs through the same plan).  With the 5,056
    frames of the linear set for every track the Hi-Fi tracks (25,280) would need repairs; with 25,280 for every
    track the bytes stay and this test cannot tell -- the host checker's warm-up check does."""
    sets, set_of, frames = M.sets_of(["stereo_hifi", "stereo_linear"]), [0, 1] * 3, [60000, 12000] * 3
    tracks = M.make_tracks(frames, sets, set_of)
    want, pos = M.expect(sets, set_of, tracks, pos=1000)
    sim.rng_pos = 1000
    chain = ntscsim.AudioChain(sets[1], sim=sim)                                 # bound: the SHORT warm-up
    assert chain.default_warmup() == 5056
    states = chain.zero_states(6)
    got = run_mixed(chain, sets, set_of, tracks, states)
    assert_tracks(got, want, states)
    assert sim.rng_pos == pos
    assert chain.track_stats(6) == [((f + 4095) // 4096, 0) for f in frames]


def test_rand_rules(sim):
    mono = T.params(["-vhs", "-vhs-hifi", "0"])                                  # mono, hiss level 39
    sets = [mono, M.PRESETS["no_hiss"](), M.PRESETS["loud_hiss"]()]
    assert sets[0].hiss_level != 0 and sets[1].hiss_level == 0 and sets[2].hiss_level not in (0, sets[0].hiss_level)
    set_of, frames = [0, 1, 2], [500, 700, 300]
    tracks = M.make_tracks(frames, sets, set_of, seed=70)
    chain = ntscsim.AudioChain(sets[0], sim=sim)
    chain.set_plan(128, 32)
    # NTSCSIM_RNG_AUTO throughout: only the hissing tracks move the position, by their own channel-samples
    want, pos = M.expect(sets, set_of, tracks, pos=1 << 33)
    sim.rng_pos = 1 << 33
    states = chain.zero_states(3)
    got = run_mixed(chain, sets, set_of, tracks, states)
    assert_tracks(got, want, states, what="auto")
    assert sim.rng_pos == pos == (1 << 33) + 500 + 2 * 300
    # explicit positions, a backward one; a position set inside the track that draws nothing; blocks without samples
    blocks = [[(200, 5000), (0, None), (300, 100)], [(1, None), (699, 77777)], [(0, 12), (300, None), (0, None)]]
    want, pos = M.expect(sets, set_of, tracks, pos=41, blocks=blocks)
    sim.rng_pos = 41
    states = chain.zero_states(3)
    got = run_mixed(chain, sets, set_of, tracks, states, blocks)
    assert_tracks(got, want, states, what="explicit")
    assert sim.rng_pos == pos == 12 + 600
    # a block without samples behind the last track still sets the position
    blocks = [None, None, [(300, None), (0, 999)]]
    want, _ = M.expect(sets, set_of, tracks, pos=7, blocks=[None, None, [(300, None)]])
    sim.rng_pos = 7
    got = run_mixed(chain, sets, set_of, tracks, None, blocks)
    assert_tracks(got, want, what="tail")
    assert sim.rng_pos == 999
    chain.set_plan(0, 0)


def test_equivalences(sim):
    """Every track on one set equals ntscsim_audio_tracks_device on the same inputs; set == -1 equals naming a copy of
    the bound parameters; n_sets == 0 is allowed."""
    ap = M.PRESETS["stereo_linear"]()
    frames = list(T.STRADDLE)
    tracks = M.make_tracks(frames, [ap], [0] * len(frames), seed=12)
    chain = ntscsim.AudioChain(ap, sim=sim)
    chain.set_plan(64, 20)
    import torch
    whole = np.concatenate(tracks)
    src = torch.from_numpy(whole).cuda()
    dst = torch.full_like(src, 0x5555)
    sim.rng_pos = 9
    old_states = chain.zero_states(len(frames))
    chain.process_tracks(T.cut(src, frames), T.cut(dst, frames), old_states)
    chain.sync()
    old, old_pos, old_stats = dst.cpu().numpy(), sim.rng_pos, chain.track_stats(len(frames))
    old_state_bytes = old_states.cpu().numpy().tobytes()
    for what, sets, set_of in (("one set", [ap], [0] * len(frames)), ("the bound set", [], [-1] * len(frames)),
                               ("both", [M.PRESETS["mono_lp"](), ap], [-1 if t % 2 else 1 for t in range(len(frames))])):
        sim.rng_pos = 9
        states = chain.zero_states(len(frames))
        got = run_mixed(chain, sets, set_of, tracks, states)
        assert (np.concatenate(got) == old).all(), what
        assert states.cpu().numpy().tobytes() == old_state_bytes, what
        assert sim.rng_pos == old_pos and chain.track_stats(len(frames)) == old_stats, what
    chain.set_plan(0, 0)


def test_states(sim):
    """Counts from non-zero starts, per track and per standard (the buzz phase follows them); two calls in sequence
    continue each track; a NULL state starts from zeros; a copied track keeps a state that is not zeros.  The ctx's own
    state and bound parameters are not touched."""
    import torch
    names = ["stereo_linear", "pal_linear", "nocomp", "loud_hiss"]
    sets, set_of, frames = M.sets_of(names), [0, 1, 2, 3, 1], [3000, 3000, 500, 1000, 700]
    counts = [3000000000, (1 << 31) + 12345, 77, 0, 5]
    tracks = M.make_tracks(frames, sets, set_of, ["music", "quiet", "music", "music", "music"], seed=9)
    chain = ntscsim.AudioChain(sets[0], sim=sim)
    chain.set_plan(256, 64)
    a = torch.from_numpy(np.ascontiguousarray(tracks[0][:700])).cuda()
    chain.process(a, torch.zeros_like(a))                                       # make the ctx's own state something
    chain.sync()
    ctx_before = chain.state
    assert any(ctx_before[0])
    # the whole tracks through the checker; the device in two calls, cut at a third
    p0 = 17
    cuts = [f // 3 for f in frames]
    draws = [sets[s].channels if sets[s].enabled and sets[s].hiss_level else 0 for s in set_of]
    first_pos, at = [], p0
    for t in range(5):
        first_pos.append(at)
        at += cuts[t] * draws[t]
    second_pos = []
    for t in range(5):
        second_pos.append(at)
        at += (frames[t] - cuts[t]) * draws[t]
    blocks = [[(cuts[t], first_pos[t]), (frames[t] - cuts[t], second_pos[t])] for t in range(5)]
    want, _ = M.expect(sets, set_of, tracks, counts=counts, pos=p0, blocks=blocks)
    states = chain.zero_states(5)
    before = [(tuple([0.0] * 30), c) for c in counts]
    before[2] = (tuple(float(i + 1) for i in range(30)), 77)                     # the copied track's: kept as it is
    for t in range(5):
        chain.set_track_state(states, t, before[t])
    sim.rng_pos = p0
    got1 = run_mixed(chain, sets, set_of, [a[:c] for a, c in zip(tracks, cuts)], states)
    assert sim.rng_pos == second_pos[0]
    got2 = run_mixed(chain, sets, set_of, [a[c:] for a, c in zip(tracks, cuts)], states)
    assert sim.rng_pos == at
    assert_tracks([np.concatenate(p) for p in zip(got1, got2)], want, states, before=before)
    assert chain.state == ctx_before
    # NULL states: from zeros at count 0
    want0, _ = M.expect(sets, set_of, tracks, pos=p0)
    sim.rng_pos = p0
    assert_tracks(run_mixed(chain, sets, set_of, tracks), want0, what="NULL states")
    # the bound parameters are still set 0's: the plain call gives what the checker gives for them
    chain.state = (tuple([0.0] * 30), 0)
    sim.rng_pos = 0
    src = torch.from_numpy(np.ascontiguousarray(tracks[0])).cuda()
    dst = torch.zeros_like(src)
    chain.process(src, dst)
    chain.sync()
    assert (dst.cpu().numpy() == A.run_checker(sets[0], tracks[0])[0]).all()
    chain.set_plan(0, 0)


def expect_by_set(sets, set_of, tracks, counts, pos):
    """M.expect for many short tracks: one run of the checker per SET (A.run_tracks_checker) instead of one per track,
    every track at the position the contract gives it -- the draws of the tracks before it."""
    first = []
    for a, s in zip(tracks, set_of):
        first.append(pos)
        if sets[s].enabled and sets[s].hiss_level:
            pos += a.size
    want = [None] * len(tracks)
    for s, ap in enumerate(sets):
        mine = [t for t in range(len(tracks)) if set_of[t] == s]
        if not mine:
            continue
        if not ap.enabled:
            for t in mine:
                want[t] = (tracks[t], None)
            continue
        res, _ = A.run_tracks_checker(ap, [tracks[t] for t in mine], [counts[t] for t in mine], 0, [[(len(tracks[t]), first[t])] for t in mine])
        for t, r in zip(mine, res):
            want[t] = r
    return want, pos


def test_sizes_past_the_thresholds(sim):
    """1100 tracks of 40 frames over 7 sets: past the 1024 cap of the y grids of k_audio_hiss and k_audio_mixed_pulses.
    Then 300 distinct sets on 300 tracks: the set table is past anything a kernel argument could hold."""
    sets = M.sets_of(M.CYCLE + ("loud_hiss",))
    n = 1100
    set_of = [(t * 3 + t // 7) % 7 for t in range(n)]
    counts = [1000 * t for t in range(n)]
    tracks = M.make_tracks([40] * n, sets, set_of, seed=5)
    want, pos = expect_by_set(sets, set_of, tracks, counts, 7)
    chain = ntscsim.AudioChain(sets[0], sim=sim)
    states = chain.zero_states(n)
    raw = np.zeros((n, 31), np.uint64)
    raw[:, 30] = counts
    import torch
    states.copy_(torch.from_numpy(raw.view(np.uint8).reshape(-1)))
    before = [(tuple([0.0] * 30), c) for c in counts]
    sim.rng_pos = 7
    got = run_mixed(chain, sets, set_of, tracks, states)
    assert_tracks(got, want, states, before=before)
    assert sim.rng_pos == pos
    assert chain.track_stats(n) == [(1, 0) if sets[s].enabled else (0, 0) for s in set_of]
    # 300 sets that differ in hiss level, channels and standard
    sets = []
    for i in range(300):
        flags = [["-vhs", "-vhs-hifi", "0"], [], ["-tvstd", "pal", "-vhs", "-vhs-hifi", "0"]][i % 3]
        sets.append(T.params(flags, hiss_level=10 + i, channels=1 + (i // 3) % 2))
    set_of = [(i * 7) % 300 for i in range(300)]
    assert sorted(set_of) == list(range(300))
    tracks = M.make_tracks([40] * 300, sets, set_of, seed=6)
    want, pos = M.expect(sets, set_of, tracks, pos=1)
    states = chain.zero_states(300)
    sim.rng_pos = 1
    got = run_mixed(chain, sets, set_of, tracks, states)
    assert_tracks(got, want, states, what="300 sets")
    assert sim.rng_pos == pos


def test_error_codes(sim):
    import torch
    lib = sim._lib
    ap = M.PRESETS["stereo_hifi"]()
    mono = M.PRESETS["mono_lp"]()
    one = (_capi.AudioMixedTrack * 1)()
    one[0].set = -1
    fresh = ntscsim.FieldSimulator(device=0)
    try:
        assert lib.ntscsim_audio_mixed_tracks_device(fresh._h, None, 0, one, 1, None) == _capi.E_ARG   # no bind
        assert lib.ntscsim_audio_mixed_tracks_host(fresh._h, None, 0, one, 1) == _capi.E_ARG
    finally:
        fresh.close()
    chain = ntscsim.AudioChain(ap, sim=sim)
    buf = torch.zeros(8192, dtype=torch.int16, device="cuda")
    out = torch.full((8192,), 0x5555, dtype=torch.int16, device="cuda")
    states = chain.zero_states(3)
    base, obase, sbase = buf.data_ptr(), out.data_ptr(), states.data_ptr()
    assert sbase % 8 == 0
    bad_size, bad_param = M.PRESETS["stereo_hifi"](), M.PRESETS["stereo_hifi"]()
    bad_size.struct_size += 8
    bad_param.channels = 3
    sets = (_capi.AudioParams * 4)(ap, mono, bad_size, bad_param)
    sim.rng_pos = 5

    def call(t0, t1=None, n=None, n_sets=4, use_sets=sets):
        """tracks given as (src, dst, samples, state, set)"""
        given = [t for t in (t0, t1) if t is not None]
        arr = (_capi.AudioMixedTrack * len(given))()
        descs = (_capi.AudioDesc * len(given))()
        for t, (src, dst, samples, state, s) in enumerate(given):
            descs[t].src, descs[t].dst, descs[t].samples, descs[t].rng_pos = src, dst, samples, _capi.RNG_AUTO
            arr[t].blocks = C.cast(C.byref(descs[t]), C.POINTER(_capi.AudioDesc))
            arr[t].n_blocks = 1
            arr[t].state = state
            arr[t].set = s
        return lib.ntscsim_audio_mixed_tracks_device(sim._h, use_sets, n_sets, arr, len(given) if n is None else n, None)

    ok0, ok1 = (base, obase, 100, sbase, 0), (base + 4096, obase + 4096, 100, sbase + chain.STATE_BYTES, 1)
    E = _capi.E_ARG
    assert lib.ntscsim_audio_mixed_tracks_device(None, sets, 4, one, 1, None) == E              # a NULL ctx
    assert call(ok0, ok1, n=-1) == E
    assert lib.ntscsim_audio_mixed_tracks_device(sim._h, sets, 4, None, 1, None) == E           # NULL tracks
    nb = (_capi.AudioMixedTrack * 1)()
    nb[0].n_blocks = 1
    assert lib.ntscsim_audio_mixed_tracks_device(sim._h, sets, 4, nb, 1, None) == E             # NULL blocks
    assert call(ok0, (None, obase + 4096, 100, None, 0)) == E                                   # NULL and odd pointers
    assert call(ok0, (base + 4096, None, 100, None, 0)) == E
    assert call(ok0, (base + 4097, obase + 4096, 100, None, 0)) == E
    assert call(ok0, (base + 4096, obase + 4097, 100, None, 0)) == E
    assert call(ok0, (base + 4096, obase + 4096, 100, sbase + chain.STATE_BYTES + 4, 0)) == E   # a state not 8-byte aligned
    assert call(ok0, (base + 4096, obase + 4096, 100, sbase, 0)) == E                           # two tracks, one state
    assert call(ok0, (base + 4096, obase + 4096, 100, sbase + 240, 0)) == E                     # overlapping states
    assert call((base, base, 100, sbase, 0)) == E                                               # in place
    assert call((base, base + 396, 100, sbase, 0)) == E                                         # dst overlaps the end of its stereo src
    assert call((base, base + 396, 100, None, 1)) == _capi.OK                                   # ... but not of a MONO src of 100 frames
    sim.sync()
    assert sim.rng_pos == 5 + 100
    buf.zero_()
    torch.cuda.synchronize()
    sim.rng_pos = 5
    assert call(ok0, (base + 4096, base + 396, 100, None, 0)) == E                              # dst overlaps the src of another track
    assert call((base + 4096, base + 396, 100, None, 0), ok0) == E
    assert call(ok0, (base + 4096, obase + 4096, 100, None, 4)) == E                            # a set outside -1 .. n_sets-1
    assert call(ok0, (base + 4096, obase + 4096, 100, None, -2)) == E
    assert call(ok0, ok1, n_sets=-1) == E
    assert call(ok0, ok1, n_sets=1) == E                                                        # set 1 of one set
    assert call(ok0, ok1, use_sets=None) == E                                                   # NULL sets that should hold something
    assert call(ok0, (base + 4096, obase + 4096, 100, None, 2)) == E                            # a wrong struct_size
    assert call(ok0, (base + 4096, obase + 4096, 100, None, 3)) == _capi.E_PARAM                # what bind refuses
    sim.sync()
    assert sim.rng_pos == 5                                                                     # a refused call draws nothing
    assert bool((out == 0x5555).all()) and not bool(buf.any()) and not bool(states.any())       # and writes nothing
    assert call(ok0, (None, None, 0, None, 1)) == _capi.OK                                      # an empty block needs no pointers
    assert lib.ntscsim_audio_mixed_tracks_device(sim._h, None, 0, None, 0, None) == _capi.OK    # no tracks at all
    assert call(ok0, ok1) == _capi.OK                                                           # sets 2 and 3 are invalid, and unnamed
    sim.sync()
    assert sim.rng_pos == 5 + 200 + 200 + 100
    s = (_capi.AudioStats * 3)()
    assert lib.ntscsim_audio_debug_track_stats(sim._h, s, 3) == E                               # the last call had two tracks
    assert lib.ntscsim_audio_debug_track_stats(sim._h, s, 2) == _capi.OK
    # the next call is exact
    sets2, set_of = [ap, mono], [0, 1]
    tracks = M.make_tracks([300, 300], sets2, set_of, seed=3)
    want, pos = M.expect(sets2, set_of, tracks, pos=5)
    sim.rng_pos = 5
    st = chain.zero_states(2)
    assert_tracks(run_mixed(chain, sets2, set_of, tracks, st), want, st)
    assert sim.rng_pos == pos


def test_host_form_and_veneer(sim):
    """mixed_tracks_host on unaligned numpy buffers, in place, with host states, equals the device call (and the
    checker); process_mixed_tracks on tensors that are not neighbours; kernel_ms after a mixed call."""
    import torch
    sets = M.sets_of(M.CYCLE)
    frames = [700, 0, 129, 2000, 300, 450, 64]
    set_of = [2, 0, 1, 0, 4, 5, 3]
    counts = [9, 0, 0, 123456789, 4, 1 << 32, 0]
    tracks = M.make_tracks(frames, sets, set_of, seed=90)
    want, pos = M.expect(sets, set_of, tracks, counts=counts, pos=2)
    chain = ntscsim.AudioChain(sets[1], sim=sim)
    chain.set_plan(128, 40)
    before = [(tuple([0.0] * 30), c) for c in counts]
    # the device call, on tensors of their own
    srcs = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in tracks]
    dsts = [torch.full_like(s, 0x5555) for s in srcs]
    states = chain.zero_states(7)
    for t in range(7):
        chain.set_track_state(states, t, before[t])
    chain.debug_time_kernels(True)
    sim.rng_pos = 2
    chain.process_mixed_tracks(sets, set_of, srcs, dsts, states)
    chain.sync()
    assert len(chain.kernel_ms()) == 3
    chain.debug_time_kernels(False)
    assert_tracks([d.cpu().numpy() for d in dsts], want, states, before=before)
    assert sim.rng_pos == pos
    dev_stats = chain.track_stats(7)
    assert [s[0] for s in dev_stats] == [6, 0, 2, 16, 0, 4, 1]
    # the host call: every track at an odd address of one byte buffer, in place, host states
    raw = np.zeros(sum(a.nbytes for a in tracks) + 1, np.uint8)
    arrays, at = [], 1
    for a in tracks:
        v = raw[at:at + a.nbytes].view(np.int16).reshape(a.shape)
        assert v.ctypes.data % 2 == 1 or a.size == 0
        v[...] = a
        arrays.append(v)
        at += a.nbytes
    host_states = np.zeros(7 * chain.STATE_BYTES, np.uint8)
    host_states.view(np.uint64).reshape(7, 31)[:, 30] = counts
    sim.rng_pos = 2
    chain.host_mixed_tracks(sets, set_of, arrays, host_states)
    assert sim.rng_pos == pos
    for t, (v, (w, _st)) in enumerate(zip(arrays, want)):
        assert (v == w).all(), "host track %d" % t
    assert host_states.tobytes() == states.cpu().numpy().tobytes()
    assert chain.track_stats(7) == dev_stats
    assert raw[0] == 0
    # two host tracks on one state are refused
    arr, trk, _keep = chain._mixed_tracks(sets, [0, 0], [(arrays[2].ctypes.data, arrays[2].ctypes.data, 0)] * 2, [host_states.ctypes.data] * 2, None)
    assert sim._lib.ntscsim_audio_mixed_tracks_host(sim._h, arr, len(sets), trk, 2) == _capi.E_ARG
    chain.set_plan(0, 0)
