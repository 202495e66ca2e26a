"""The CPU half of tests/test_audio_limits_gpu.py: the layouts really cross the thresholds they are meant for, the plans
of the mixed-repair tests meet their condition on the HOST plan (audio_run_planned / cass_run_planned), and the additions
to the checkers (`plan` with the repaired segments, `tracks`) say what the modes they lean on say."""
import numpy as np

import _audio_limits as M
import _audio_ref as A
import _audio_tracks as T
import _cass_ref as CR


def test_call_lists_are_what_the_docstrings_say():
    calls = M.packet_calls()
    assert len(calls) >= 12 and sum(1 for c in calls if M.frames_of([c])) >= 12 and M.frames_of(calls) == 22903 <= 40000
    big = [i for i, c in enumerate(calls) if M.frames_of([c]) == 12000][0]
    assert all(0 < M.frames_of([c]) <= 4097 for c in calls[big - 2:big])
    many = [i for i, c in enumerate(calls) if len(c) == 64][0]
    assert all(len(c) == 1 for c in calls[:many])
    tape = M.tape_calls()
    assert [M.frames_of([c]) for c in tape[1:5]] == [1, 2, 3, 1] and [M.frames_of([c]) for c in tape[7:13]] == [5, 7, 10, 20, 15, 3]
    assert M.frames_of([tape[13]]) == 12000


def test_many_blocks_layout():
    blocks = M.many_blocks()
    live = [b for b in blocks if b[0]]
    assert len(live) == 1500 > M.HISS_GRID_Y and all(1 <= n <= 5 for n, _ in live) and {n for n, _ in live} == {1, 2, 3, 4, 5}
    assert sum(1 for n, _ in blocks if n == 0) == 5
    given = [(i, p) for i, (n, p) in enumerate(blocks) if p is not None and n]
    assert len(given) == 15 and sum(1 for i, _ in given if i > M.HISS_GRID_Y) >= 4      # positions behind the stride, too
    first, _ = M.first_draws(blocks, 1, 7)
    steps = [first[i] - first[i - 1] for i, _ in given]
    assert sum(1 for s in steps if s < 0) >= 5 and sum(1 for s in steps if abs(s) > (1 << 33) - (1 << 20)) >= 8
    # a block without frames sets the position of the block behind it
    i = [i for i, (n, p) in enumerate(blocks) if n == 0 and p is not None][0]
    assert first[i + 1] == blocks[i][1] and blocks[i + 1][1] is None
    # 40 tracks of unequal runs hold them all, in order
    parts = M.spread(blocks, 40)
    assert len(parts) == 40 and [b for p in parts for b in p] == blocks and len({len(p) for p in parts}) > 2 and all(sum(n for n, _ in p) for p in parts)


def test_boundary_blocks_layout():
    blocks = M.boundary_blocks()
    assert sum(n for n, _ in blocks) == 140000
    first, end = M.first_draws(blocks, 1, 0)
    gaps = [b - a for a, b in zip(first, first[1:])]
    S = M.HISS_STEP_MAX
    assert gaps[:6] == [0, 1, S - 1, S, S + 1, -1]
    assert blocks[7] == (S, None) and gaps[7] == S and blocks[9] == (S + 1, None) and gaps[9] == S + 1   # RNG_AUTO behind 65536 / 65537 draws
    assert end == first[6] + 140000 - 6 * 300


def test_mixed_plans_meet_the_condition():
    ap, a = M.mixed_audio_case()
    (segs, rep), which = A.plan(ap, a, M.MIXED_SEG, M.MIXED_AUDIO["warmup"], rng_pos=M.MIXED_AUDIO["rng_pos"])
    assert segs == 32 and rep == len(which) and A.mixed_repairs(segs, which), which
    assert ap.highpass_hz == 100 and 1000 <= M.MIXED_AUDIO["warmup"] < 5056     # marginal: under the default warm-up of 100 Hz
    cp, c = M.mixed_cass_case()
    st, front, back = CR.plan(cp, c, M.MIXED_SEG, M.MIXED_CASS["front"], M.MIXED_CASS["back"], rng_pos=M.MIXED_CASS["rng_pos"])
    assert st == (32, len(front), len(back)) and A.mixed_repairs(32, front) and A.mixed_repairs(32, back), (front, back)
    assert st == CR.plan_stats(cp, c, M.MIXED_SEG, M.MIXED_CASS["front"], M.MIXED_CASS["back"], rng_pos=M.MIXED_CASS["rng_pos"])
    ap, tracks, pos = M.mixed_tracks_case()
    plans = [A.plan(ap, t, M.MIXED_SEG, M.MIXED_TRACKS["warmup"], rng_pos=p) for t, p in zip(tracks, pos)]
    assert plans[0][0] == (12, 0) and plans[2][0] == (12, 0) and A.mixed_repairs(32, plans[1][1]), plans


def test_mixed_repairs_condition():
    assert A.mixed_repairs(8, [3]) and A.mixed_repairs(8, [2, 3, 6])
    assert not A.mixed_repairs(8, []) and not A.mixed_repairs(8, list(range(1, 8)))
    assert not A.mixed_repairs(8, [7]) and not A.mixed_repairs(8, [5, 6, 7])     # nothing is accepted behind a repair


def test_plan_mode_counts_what_planned_asserts():
    """W = 0 on input that is not silent repairs every segment but the first; the default warm-up repairs none."""
    ap = T.PRESETS["stereo_hifi"]()
    a = A.make_input("music", 3000, 2, 6)
    assert A.plan(ap, a, 256, 0) == ((12, 11), list(range(1, 12)))
    assert A.plan(ap, a, 256, 30000) == ((12, 0), [])
    assert A.plan_stats(T.PRESETS["nocomp"](), a, 256, 0) == (0, 0)


def test_tracks_mode_is_the_serial_mode_per_track():
    ap = T.PRESETS["mono_lp"]()
    frames = [37, 0, 200, 1]
    tracks = T.cut(T.make_tracks(frames, 1, seed=11), frames)
    counts = [0, 5, 3000000000, 100003]
    blocks = [[(30, 900), (0, None), (7, 5)], [(0, 77)], None, [(1, 1 << 33)]]
    got, pos = A.run_tracks_checker(ap, tracks, counts=counts, pos=3, blocks=blocks)
    at = 3
    for t, a in enumerate(tracks):
        if len(a) == 0:
            assert got[t][1] == (tuple([0.0] * 30), counts[t]) and len(got[t][0]) == 0
            at = 77
            continue
        spec = "blocks=" + A.block_spec(blocks[t]) if blocks[t] is not None else 0
        want, st, at = A.run_checker(ap, a, count0=counts[t], rng_pos=at, block=spec)
        assert (got[t][0] == want).all() and got[t][1][1] == st[1] and (A.state_bits(got[t][1][0]) == A.state_bits(st[0])).all(), t
    assert pos == at == (1 << 33) + 1


def test_the_new_checker_modes_under_sanitizers():
    """`plan` and `tracks` of the checkers built with the address and undefined-behaviour sanitizers, run as the programs
    they are, say what the plain builds say."""
    ap, a = M.mixed_audio_case()
    args = (ap, a[:3000], M.MIXED_SEG, 700)
    assert A.plan(*args, rng_pos=5, build="sanitized") == A.plan(*args, rng_pos=5)
    cp, c = M.mixed_cass_case()
    cargs = (cp, c[:3000], M.MIXED_SEG, 700, 20)
    assert CR.plan(*cargs, rng_pos=5, build="sanitized") == CR.plan(*cargs, rng_pos=5)
    mono = T.PRESETS["mono_lp"]()
    parts = M.spread(M.many_blocks(), 40)[:6]
    frames = [sum(n for n, _ in p) for p in parts]
    tracks = T.cut(T.make_tracks(frames, 1, seed=73), frames)
    plain, pos = A.run_tracks_checker(mono, tracks, counts=list(range(6)), pos=7, blocks=parts)
    san, spos = A.run_tracks_checker(mono, tracks, counts=list(range(6)), pos=7, blocks=parts, build="sanitized")
    assert pos == spos and all((x[0] == y[0]).all() and x[1] == y[1] for x, y in zip(plain, san))
