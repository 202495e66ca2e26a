"""Audio calls IN FLIGHT: ntscsim_audio_device, ntscsim_cass_device and ntscsim_audio_tracks_device issued back to back
with nothing that waits for the device between them, as the tools issue a packet per thousand frames -- the record-slot
ring and its waits, the growth of the scratch planes and of the tilt staging under queued launches, the host's copy of
the cassette's sample count, the states and the FIR history carried through device memory alone, and the calls that
promise to wait for work in flight (csrc/ntsc_stage.hpp, csrc/ntsc_audio.hip, csrc/ntsc_cass.hip).

The expectation is the serial host chain (A.run_checker / C.run_checker with a blocks= spec where the stream is cut,
A.run_tracks_checker per track), never the code under test; the chain is exact arithmetic, so the tolerance is zero:
bytes, state bits with the FIR history, the rand() position and, where stated, the repair counts.

Every test makes its own FieldSimulator: scratch and slot capacities start small only on a fresh ctx, and growing them
while launches are queued is the point.  All inputs are uploaded and all outputs allocated first; the calls go to a
stream of their own (torch's default stream would be waited for by FieldSimulator._torch_stream), then ONE wait.
Whether a call really is still queued when the next is issued is up to the machine: these tests pass if the waits are
right, and they cannot show that a missing wait would fail."""
import contextlib

import numpy as np
import pytest

import _audio_limits as M
import _audio_ref as A
import _audio_tracks as T
import _cass_ref as CR
import _libs as L
import ntscsim
import test_audio_gpu as TA
import test_audio_tracks_gpu as TT
import test_cass_gpu as TC
from ntscsim import _capi

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def fresh(params=None):
    fs = ntscsim.FieldSimulator(device=0) if params is None else ntscsim.FieldSimulator(params=params, device=0)
    try:
        yield fs
    finally:
        fs.close()


def upload(a, fill=0x5555):
    import torch
    src = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return src, torch.full_like(src, fill)


def side_streams(n=1):
    """n streams, created once everything uploaded so far is on the device"""
    import torch
    torch.cuda.synchronize()
    return [torch.cuda.Stream() for _ in range(n)]


def settle():
    """what torch's default stream was given (fills, uploads) is on the device before a side stream touches it"""
    import torch
    torch.cuda.synchronize()


def issue(chain, src, dst, calls, streams):
    """the calls on consecutive slices of src / dst; with two streams they alternate, each call behind the one before
    it through an event (wait_stream).  Nothing here waits on the host."""
    at = 0
    for i, blocks in enumerate(calls):
        n = sum(b[0] for b in blocks)
        st = streams[i % len(streams)]
        if len(streams) > 1:
            st.wait_stream(streams[(i - 1) % len(streams)])
        chain.process(src[at:at + n], dst[at:at + n], blocks, stream=st.cuda_stream)
        at += n
    assert at == src.shape[0]


def finish(fs, streams, src, dst, a):
    """the one wait; the output as numpy"""
    import torch
    for st in streams:
        st.synchronize()
    fs.sync()
    assert torch.equal(src.cpu(), torch.from_numpy(np.ascontiguousarray(a))), "a call wrote its source"
    return dst.cpu().numpy()


def spec_of(calls):
    return "blocks=" + A.block_spec([b for c in calls for b in c])


frames_of = M.frames_of


# ---------------------------------------------------------------------------------------------- A1, A2: packets
@pytest.mark.parametrize("plan", [(0, 0), (64, 20)], ids=["default_plan", "plan_64_20"])
@pytest.mark.parametrize("preset", ["stereo_hifi", "stereo_linear", "mono_lp"])
def test_packets_through_the_audio_chain(preset, plan):
    ap = T.PRESETS[preset]()
    calls = M.packet_calls()
    a = A.make_input("music", frames_of(calls), ap.channels, 61)
    want, st, pos = A.run_checker(ap, a, rng_pos=11, block=spec_of(calls))
    with fresh() as fs:
        chain = ntscsim.AudioChain(ap, sim=fs)
        chain.set_plan(*plan)
        fs.rng_pos = 11
        src, dst = upload(a)
        streams = side_streams()
        issue(chain, src, dst, calls, streams)
        got = finish(fs, streams, src, dst, a)
        TA.assert_same(chain, got, want, st, "%s plan %s" % (preset, plan))
        assert fs.rng_pos == pos
        assert chain.stats()[0] == (1152 + (plan[0] or 4096) - 1) // (plan[0] or 4096)


TAPE_SETS = {
    "default": ([], 0),
    "bad_deck_deemph": (["-preset", "3", "-deemphasis", "1"], 0),
    "bad_deck_mono_both": (["-preset", "3", "-mono", "-preemphasis", "1", "-deemphasis", "1"], 0),
    "bad_deck_deemph_count_3e9": (["-preset", "3", "-deemphasis", "1"], 3000000000),
}


@pytest.mark.parametrize("which", sorted(TAPE_SETS))
def test_packets_through_the_cassette(which):
    flags, count0 = TAPE_SETS[which]
    cp = _capi.make_cass_params(flags)
    assert cp.taps == (57 if "-preset" in flags else 8)
    calls = M.tape_calls()
    a = A.make_input("music", frames_of(calls), 2, 62)
    want, st, pos = CR.run_checker(cp, a, count0=count0, rng_pos=11, block=spec_of(calls))
    if count0:
        zero, _, _ = CR.run_checker(cp, a, count0=0, rng_pos=11, block=spec_of(calls))
        assert int((want != zero).sum()) > 100                                  # the host's count is audible
    with fresh() as fs:
        chain = ntscsim.Cassette(cp, sim=fs)
        if count0:
            chain.state = (tuple([0.0] * 28), count0, ())
        fs.rng_pos = 11
        src, dst = upload(a)
        streams = side_streams()
        issue(chain, src, dst, calls, streams)
        got = finish(fs, streams, src, dst, a)
        TC.assert_same(chain, got, want, st, which)
        assert fs.rng_pos == pos


# ---------------------------------------------------------------------------------------------- A3: tracks
def test_tracks_prefix_rest_single_stream_and_many_tracks():
    """A prefix of every track, then the rest, on one state tensor; a single-stream call; a call of 600 tracks -- four
    calls, no wait.  (600, not 300: the first tracks call leaves room for 519 tracks' stats, so only more than that
    makes track_stats grow.)"""
    import torch
    ap = T.PRESETS["stereo_linear"]()
    assert ap.hiss_level != 0 and ap.buzz != 0
    frames = [700, 1, 300, 64, 0, 1300]
    counts = [0, 3000000000, 17, 100003, 5, 200006]
    cuts = [f // 3 for f in frames]
    tracks = T.cut(T.make_tracks(frames, 2, seed=33), frames)
    single = A.make_input("music", 900, 2, 34)
    nbig = 600
    big_frames = [1 + t % 3 for t in range(nbig)]
    big = T.cut(T.make_tracks(big_frames, 2, seed=35), big_frames)
    # draws in call order
    p0 = 23
    pos1, at = [], p0
    for c in cuts:
        pos1.append(at)
        at += 2 * c
    pos2 = []
    for f, c in zip(frames, cuts):
        pos2.append(at)
        at += 2 * (f - c)
    p_single = at
    want, _ = A.run_tracks_checker(ap, tracks, counts=counts, pos=p0, blocks=[[(c, a1), (f - c, a2)] for f, c, a1, a2 in zip(frames, cuts, pos1, pos2)])
    want_single, st_single, p_big = A.run_checker(ap, single, rng_pos=p_single)
    want_big, p_end = A.run_tracks_checker(ap, big, pos=p_big)
    with fresh() as fs:
        chain = ntscsim.AudioChain(ap, sim=fs)
        chain.set_plan(64, 20)
        raw = np.zeros((len(frames), 31), np.uint64)
        raw[:, 30] = counts
        states = torch.from_numpy(raw.view(np.uint8).reshape(-1)).cuda()
        big_states = chain.zero_states(nbig)
        src, dst = upload(np.concatenate(tracks))
        ssrc, sdst = upload(single)
        bsrc, bdst = upload(np.concatenate(big))
        tsrc, tdst = T.cut(src, frames), T.cut(dst, frames)
        fs.rng_pos = p0
        (st,) = side_streams()
        chain.process_tracks([x[:c] for x, c in zip(tsrc, cuts)], [x[:c] for x, c in zip(tdst, cuts)], states, stream=st.cuda_stream)
        chain.process_tracks([x[c:] for x, c in zip(tsrc, cuts)], [x[c:] for x, c in zip(tdst, cuts)], states, stream=st.cuda_stream)
        chain.process(ssrc, sdst, stream=st.cuda_stream)
        chain.process_tracks(T.cut(bsrc, big_frames), T.cut(bdst, big_frames), big_states, stream=st.cuda_stream)
        st.synchronize()
        fs.sync()
        assert fs.rng_pos == p_end
        TT.assert_tracks([np.array(x) for x in T.cut(dst.cpu().numpy(), frames)], want, states, what="prefix and rest")
        TA.assert_same(chain, sdst.cpu().numpy(), want_single, st_single, "the single stream between the tracks calls")
        TT.assert_tracks([np.array(x) for x in T.cut(bdst.cpu().numpy(), big_frames)], want_big, what="600 tracks")
        got_states = big_states.cpu().numpy().view(np.uint64).reshape(nbig, 31)
        exp_states = np.array([list(A.state_bits(s[0])) + [s[1]] for _, s in want_big], np.uint64)
        assert (got_states == exp_states).all(), "600 tracks: states of tracks %s" % np.nonzero((got_states != exp_states).any(axis=1))[0][:10]
        assert [s[0] for s in chain.track_stats(nbig)] == [1] * nbig


# ---------------------------------------------------------------------------------------------- A4: the calls that wait
def test_audio_calls_that_promise_to_wait():
    ap = T.PRESETS["stereo_linear"]()
    a1, a2 = A.make_input("music", 6000, 2, 41), A.make_input("loud", 3000, 2, 42)
    want1, st1, pos1 = A.run_checker(ap, a1, rng_pos=9)
    want2, st2, pos2 = A.run_checker(ap, a2, rng_pos=pos1)
    with fresh() as fs:
        chain = ntscsim.AudioChain(ap, sim=fs)
        chain.set_plan(256, 0)
        src1, dst1 = upload(a1)
        src2, dst2 = upload(a2)
        dst1b = dst1.clone()
        (st,) = side_streams()
        # a state getter directly behind an enqueued call
        fs.rng_pos = 9
        chain.process(src1, dst1, stream=st.cuda_stream)
        vals, count = chain.state
        assert count == st1[1] and (A.state_bits(vals) == A.state_bits(st1[0])).all()
        # stats directly behind an enqueued call: that call's numbers
        chain.reset()
        fs.rng_pos = 9
        chain.process(src1, dst1b, stream=st.cuda_stream)
        assert chain.stats() == A.plan_stats(ap, a1, 256, 0, rng_pos=9) == (24, 23)
        assert (dst1b.cpu().numpy() == want1).all()
        # reset() directly behind an enqueued call, then a second stream from zeros
        chain.reset()
        dst1.fill_(0x5555)
        settle()
        fs.rng_pos = 9
        chain.process(src1, dst1, stream=st.cuda_stream)
        chain.reset()
        chain.process(src2, dst2, stream=st.cuda_stream)
        st.synchronize()
        fs.sync()
        assert (dst1.cpu().numpy() == want1).all(), "reset() disturbed the call before it"
        TA.assert_same(chain, dst2.cpu().numpy(), want2, st2, "the stream behind reset()")
        assert fs.rng_pos == pos2
        # a fresh bind directly behind an enqueued call
        chain.reset()
        dst1.fill_(0x5555)
        settle()
        fs.rng_pos = 9
        chain.process(src1, dst1, stream=st.cuda_stream)
        other = ntscsim.AudioChain(T.PRESETS["mono_lp"](), sim=fs)
        st.synchronize()
        fs.sync()
        assert (dst1.cpu().numpy() == want1).all(), "a bind disturbed the call before it"
        assert other.state == (tuple([0.0] * 30), 0)


def test_cassette_calls_that_promise_to_wait():
    cp = _capi.make_cass_params(["-preset", "3", "-deemphasis", "1"])
    a1, a2 = A.make_input("music", 6000, 2, 43), A.make_input("loud", 3000, 2, 44)
    want1, st1, pos1 = CR.run_checker(cp, a1, rng_pos=9)
    want2, st2, pos2 = CR.run_checker(cp, a2, rng_pos=pos1)
    with fresh() as fs:
        chain = ntscsim.Cassette(cp, sim=fs)
        chain.set_plan(256, 0, 0)
        src1, dst1 = upload(a1)
        src2, dst2 = upload(a2)
        dst1b = dst1.clone()
        (st,) = side_streams()
        fs.rng_pos = 9
        chain.process(src1, dst1, stream=st.cuda_stream)
        vals, count, hist = chain.state                                        # a state getter directly behind an enqueued call
        assert count == st1[1] and (TC.bits(vals) == st1[0]).all() and (TC.bits(hist).reshape(-1, 2) == st1[2]).all()
        chain.reset()
        fs.rng_pos = 9
        chain.process(src1, dst1b, stream=st.cuda_stream)
        stats = chain.stats()
        assert stats == CR.plan_stats(cp, a1, 256, 0, 0, rng_pos=9) and stats[0] == 24 and stats[1] == 23
        assert (dst1b.cpu().numpy() == want1).all()
        chain.reset()
        dst1.fill_(0x5555)
        settle()
        fs.rng_pos = 9
        chain.process(src1, dst1, stream=st.cuda_stream)
        chain.reset()
        chain.process(src2, dst2, stream=st.cuda_stream)
        st.synchronize()
        fs.sync()
        assert (dst1.cpu().numpy() == want1).all(), "reset() disturbed the call before it"
        TC.assert_same(chain, dst2.cpu().numpy(), want2, st2, "the stream behind reset()")
        assert fs.rng_pos == pos2
        chain.reset()
        dst1.fill_(0x5555)
        settle()
        fs.rng_pos = 9
        chain.process(src1, dst1, stream=st.cuda_stream)
        other = ntscsim.Cassette(_capi.make_cass_params([]), sim=fs)
        st.synchronize()
        fs.sync()
        assert (dst1.cpu().numpy() == want1).all(), "a bind disturbed the call before it"
        assert other.state == (tuple([0.0] * 28), 0, tuple([(0.0, 0.0)] * 7))


# ---------------------------------------------------------------------------------------------- A5: two streams
def test_two_streams_ordered_by_events():
    """include/ntscsim.h allows "one stream, or events between streams": the packets alternate between two streams,
    each call waiting for the other stream's last; the result is the one stream's."""
    ap = T.PRESETS["mono_lp"]()
    cp = _capi.make_cass_params(["-preset", "3", "-deemphasis", "1"])
    calls, tape = M.packet_calls(), M.tape_calls()
    a = A.make_input("music", frames_of(calls), 1, 63)
    c = A.make_input("music", frames_of(tape), 2, 64)
    want_a, st_a, pos_a = A.run_checker(ap, a, rng_pos=11, block=spec_of(calls))
    want_c, st_c, pos_c = CR.run_checker(cp, c, rng_pos=pos_a, block=spec_of(tape))
    with fresh() as fs:
        audio = ntscsim.AudioChain(ap, sim=fs)
        cass = ntscsim.Cassette(cp, sim=fs)
        fs.rng_pos = 11
        asrc, adst = upload(a)
        csrc, cdst = upload(c)
        streams = side_streams(2)
        issue(audio, asrc, adst, calls, streams)
        issue(cass, csrc, cdst, tape, streams)
        got_a = finish(fs, streams, asrc, adst, a)
        got_c = cdst.cpu().numpy()
        TA.assert_same(audio, got_a, want_a, st_a, "audio on two streams")
        TC.assert_same(cass, got_c, want_c, st_c, "cassette on two streams")
        assert fs.rng_pos == pos_c


# ---------------------------------------------------------------------------------------------- A6: fields and audio
def test_fields_and_audio_in_flight_on_one_ctx():
    """tests/test_audio_gpu.py's test_fields_and_audio_share_the_stream (fields, an audio block, fields, an audio
    block) with no wait until the end."""
    import torch
    w, h = 96, 32
    p = L.make_params(["-vhs"])
    ap = TA.params(["-vhs"])
    frames = [L.noise_frame(w, h, 77 + i) for i in range(2)]
    jobs = [(k // 2, k, (k & 1) ^ 1, k) for k in range(4)]
    exp = np.zeros((4, h, w, 4), np.uint8)
    o = L.OracleStream(p)
    a = A.make_input("music", 1601 + 1152, 2, 4)
    for (si, di, field, fieldno) in jobs[:2]:
        o.field(exp[di], frames[si], field, fieldno)
    p_audio1 = o.rng_pos
    _, _, behind = A.run_checker(ap, a[:1601], rng_pos=p_audio1)
    o.skip(behind - p_audio1)
    for (si, di, field, fieldno) in jobs[2:]:
        o.field(exp[di], frames[si], field, fieldno)
    p_audio2 = o.rng_pos
    want, st, pos = A.run_checker(ap, a, block="blocks=1601:%d,1152:%d" % (p_audio1, p_audio2))
    with fresh(p) as fs:
        chain = ntscsim.AudioChain(ap, sim=fs)
        src = torch.from_numpy(np.stack(frames)).cuda()
        dst = torch.zeros((4, h, w, 4), dtype=torch.uint8, device="cuda")
        asrc, adst = upload(a)
        (stream,) = side_streams()
        with torch.cuda.stream(stream):
            fs.fields(src, dst, jobs[:2])
            chain.process(asrc[:1601], adst[:1601])
            fs.fields(src, dst, jobs[2:])
            chain.process(asrc[1601:], adst[1601:])
        stream.synchronize()
        fs.sync()
        assert fs.rng_pos == pos
        TA.assert_same(chain, adst.cpu().numpy(), want, st)
        assert (dst.cpu().numpy() == exp).all()
