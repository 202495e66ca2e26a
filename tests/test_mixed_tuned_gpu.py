"""ntscsim_mixed_fields_device under ntscsim_set_mixed_forms(NTSCSIM_MIXED_TUNED): sets of the default / -vhs preset families
run the hand-tuned kernel forms (csrc/ntsc_mixed_fast.hip) in the one call, every other set the generic mixed kernels.  The
yardstick is the CPU oracle, as in tests/test_mixed_fields_gpu.py: per descriptor, that set's parameters from that
descriptor's rand() position; whole destination buffers byte for byte, tolerance 0.  The kernel lists are DERIVED from
what ntscsim_fields_device picks for each set on a context of its own (tests/_mixed_tuned.py), not written down."""
import ctypes as C
import random

import numpy as np
import pytest

import _libs as L
import _mixed_tuned as T
import ntscsim
import test_mixed_fields_gpu as G
from ntscsim import _capi

pytestmark = pytest.mark.gpu

FILL = T.FILL
FLAGS = G.FLAGS
desc = T.desc
LUMA_RING_BYTES = 4096


def family_sets():
    sets, descs = G.family_call()
    return sets, descs


# ---------------------------------------------------------------------------------------------- 1
def test_every_switch_family_in_one_tuned_call():
    """This is the test that fails without the feature: the hand-tuned forms must be the ones that run."""
    sets, descs = family_sets()
    names, _ = T.tuned_vs_oracle(sets, descs, 96, 32, 4, len(descs))
    assert names == T.derived_names(sets, 96, 32)
    for k in ("k_mixed_encode_fast<double>", "k_mixed_decode_fast<false,double>", "k_mixed_decode_fast<true,double>",
              "k_mixed_decode_fast_sv<double>"):
        assert k in names, names
    # the family holds sets of every kind the rule leaves to the generic kernels, too
    assert "k_mixed_encode<double>" in names and "k_mixed_decode<true,true,double>" in names


@pytest.mark.parametrize("case", [c for c in G.cases.CASES], ids=[c[0] for c in G.cases.CASES])
def test_the_rule_is_the_single_set_launchers_on_every_row(case):
    """ntscsim_debug_mixed_form_of (what the CPU tests sweep) against the kernels ntscsim_fields_device really launches"""
    p = L.make_params(case[1])
    e, d = C.c_int(-1), C.c_int(-1)
    assert ntscsim.lib().ntscsim_debug_mixed_form_of(C.byref(p), 96, 32, 2, 1, 0, C.byref(e), C.byref(d)) == _capi.OK
    enc = ["k_mixed_encode<double>", "k_mixed_encode_fast<double>", "k_mixed_encode_fast_pre<double>"][e.value]
    dec = ([g % "double" for g in T.GENERIC_ORDER] + [t.replace("k_", "k_mixed_", 1) % "double" for t in T.TUNED_DEC])[d.value]
    assert T.derived_names([p], 96, 32) == ["k_mixed_setup", enc, dec]


# ---------------------------------------------------------------------------------------------- 2
REGIME_SETS = [["-vhs"], ["-vhs", "-vhs-speed", "lp"], ["-vhs", "-vhs-speed", "ep"], ["-vhs", "-vhs-svideo", "1"], []]


@pytest.mark.parametrize("w,h", [(28, 10), (32, 10), (36, 10), (40, 10), (44, 10), (36, 130)])
def test_rows_of_every_regime_in_one_launch(w, h):
    """SP, LP and EP (chroma delays 9, 12, 14: the grouped row ends start at W >= 2 d + 12, S-Video's loop at 2 d + 5) with
    S-Video and the default set: widths on both sides of every threshold, so one launch of the composite -vhs form holds
    rows with the luma ring, grouped rows without it and one-position rows; 36 x 130: groups of more than one block."""
    sets = [L.make_params(f) for f in REGIME_SETS]
    single_lds = []
    for order in (list(range(5)), list(range(4, -1, -1))):
        descs = []
        for s in order:
            for k in range(2):
                descs.append(desc(s, len(descs) % 3, len(descs), (k + s) & 1, 5 * s + k))
        names, lds = T.tuned_vs_oracle(sets, descs, w, h, 3, len(descs), seed=w + h)
        assert names == T.derived_names(sets, w, h)
        assert names.count("k_mixed_decode_fast<true,double>") == 1 and "k_mixed_decode_fast_sv<double>" in names
        single_lds.append(lds)
    # the launch asks for the ring exactly when one of its groups runs it: the SP set's own single-set launch tells
    sp = ntscsim.FieldSimulator(params=sets[0])
    torch = T.torch_mod()
    src = torch.from_numpy(np.stack([L.noise_frame(w, h, 1)])).cuda()
    dst = torch.zeros((1, h, w, 4), dtype=torch.uint8, device="cuda")
    sp.fields(src, dst, [(0, 0, 1, 0)])
    want = sp.last_decoder_lds()
    sp.sync()
    sp.close()
    assert single_lds == [want, want]
    if w == 36:
        assert want == LUMA_RING_BYTES


# ---------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("h", [125, 126, 127, 128, 129, 130, 33])
def test_block_edges(h):
    """As the generic call's: Lslot on both sides of 63 and 64, groups of 1, 2 and 3 fields in both orders.  The vertical
    blend's halo at a group's first decoder block is what shows."""
    sets = [L.make_params(["-vhs"]), L.make_params(FLAGS["vhs_noblend"]), L.make_params([])]
    for order in ([0, 1, 2], [2, 1, 0]):
        descs = []
        for s in order:
            for k in range(s + 1):
                descs.append(desc(s, len(descs) % 3, len(descs), (k + s) & 1, 7 * s + k))
        names, _ = T.tuned_vs_oracle(sets, descs, 64, h, 3, len(descs), seed=h)
        assert names == ["k_mixed_setup", "k_mixed_encode_fast<double>", "k_mixed_decode_fast<false,double>",
                         "k_mixed_decode_fast<true,double>"]


# ---------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("h", [32, 36])
def test_head_switching_away_from_row_0_of_the_plane(h):
    """A first group of one field (16 or 18 rows), so that the next group starts at row 64; then the sets whose head switch
    displaces rows inside the frame, and PAL (the wrap-around form), each of them once as the last group of the call.  A
    descriptor based at the group's first row, or a wrong byte offset, reads a neighbour's samples where the reference has 0."""
    hs = ["hs_pos", "hs_neg", "hs_nonoise", "vhs_pal"]
    sets = [L.make_params([])] + [L.make_params(FLAGS[n]) for n in hs]
    for rot in range(4):
        order = [0] + [1 + (k + rot) % 4 for k in range(4)]
        descs = [desc(0, 0, 0, 1, 0)]
        for s in order[1:]:
            for k in range(2):
                descs.append(desc(s, len(descs) % 3, len(descs), (k + s) & 1, 9 * s + k))
        names, _ = T.tuned_vs_oracle(sets, descs, 96, h, 3, len(descs), seed=h + rot)
        assert names == T.derived_names(sets, 96, h)
        assert "k_mixed_decode_fast<true,double,true>" in names


# ---------------------------------------------------------------------------------------------- 5
def test_fallbacks_give_todays_list():
    sets, descs = family_sets()
    today = T.generic_names(sets)
    for pad in (1, 3):                                   # unaligned linesizes somewhere in the call: no hand-tuned form
        names, _ = T.tuned_vs_oracle(sets, descs, 96, 32, 4, len(descs), pad=pad)
        assert names == today
    names, _ = T.tuned_vs_oracle(sets, descs, 96, 32, 4, len(descs), prepare=lambda s: s.debug_force_generic(True))
    assert names == today
    names, _ = T.tuned_vs_oracle(sets, descs, 96, 32, 4, len(descs), prepare=lambda s: s.debug_no_fast_decode(1))
    assert names == today
    names, _ = T.tuned_vs_oracle(sets, descs, 96, 32, 4, len(descs), prepare=lambda s: s.set_mixed_forms(False))
    assert names == today
    assert today == ["k_mixed_setup", "k_mixed_encode<double>", "k_mixed_decode<false,false,double>",
                     "k_mixed_decode<true,true,double>", "k_mixed_decode<true,false,double>"]


def test_the_switch_takes_two_values():
    sim = ntscsim.FieldSimulator()
    lib = sim._lib
    assert lib.ntscsim_set_mixed_forms(sim._h, 2) == _capi.E_ARG and lib.ntscsim_set_mixed_forms(sim._h, -1) == _capi.E_ARG
    assert lib.ntscsim_set_mixed_forms(None, 1) == _capi.E_ARG
    assert lib.ntscsim_set_mixed_forms(sim._h, 1) == _capi.OK and lib.ntscsim_set_mixed_forms(sim._h, 0) == _capi.OK
    sim.close()


def test_the_single_set_call_keeps_its_kernels_after_a_tuned_call():
    torch = T.torch_mod()
    w, h, n = 96, 32, 4
    p = L.make_params(["-vhs"])
    frames = [L.noise_frame(w, h, 0x1234567 + i) for i in range(n // 2)]
    jobs = [(k // 2, k, (k & 1) ^ 1, k) for k in range(n)]
    src_t = torch.from_numpy(np.stack(frames)).cuda()
    fresh = ntscsim.FieldSimulator(params=p)
    d0 = torch.zeros((n, h, w, 4), dtype=torch.uint8, device="cuda")
    fresh.fields(src_t, d0, jobs)
    today, lds_today = fresh.last_kernels(), fresh.last_decoder_lds()
    fresh.sync()
    fresh.close()

    sim = ntscsim.FieldSimulator(params=p)
    sim.set_mixed_forms(True)
    sets, descs = family_sets()
    scratch_t = torch.zeros((len(descs), h, w, 4), dtype=torch.uint8, device="cuda")
    src4 = torch.from_numpy(np.stack([L.noise_frame(w, h, 0x2345678 + j) for j in range(4)])).cuda()
    sim.run_mixed_descs(sets, G.build(sim, descs, src4, scratch_t), w, h)
    assert "k_mixed_decode_fast<true,double>" in sim.last_kernels()
    start = sim.rng_pos
    dst_t = torch.zeros((n, h, w, 4), dtype=torch.uint8, device="cuda")
    sim.fields(src_t, dst_t, jobs)
    assert sim.last_kernels() == today and sim.last_decoder_lds() == lds_today
    sim.sync()
    got = dst_t.cpu().numpy()
    sim.close()
    exp = np.zeros((n, h, w, 4), np.uint8)
    o = L.OracleStream(p)
    o.skip(start)
    for (si, di, field, fieldno) in jobs:
        o.field(exp[di], frames[si], field, fieldno)
    assert np.array_equal(got, exp)


# ---------------------------------------------------------------------------------------------- 6
def test_fast32_and_float_modes_equal_the_generic_call():
    """The existing suite holds every float form to the fast32 model byte for byte, so the tuned and the generic call of
    one mode must agree; FLOAT goes on running the FAST32 forms in a mixed call."""
    torch = T.torch_mod()
    w, h = 96, 32
    sets, descs = family_sets()
    src_t = torch.from_numpy(np.stack([L.noise_frame(w, h, 0x2345678 + j) for j in range(4)])).cuda()
    want = T.derived_names(sets, w, h, rt="float", mode=_capi.MODE_FAST32)
    assert all("float" in k for k in want[1:]) and "k_mixed_decode_fast<true,float>" in want and \
        "k_mixed_encode_fast<float>" in want and "k_mixed_decode_fast_sv<float>" in want
    out = {}
    for mode in (_capi.MODE_FAST32, _capi.MODE_FLOAT):
        for tuned in (True, False):
            dst_t = torch.full((len(descs), h, w, 4), FILL, dtype=torch.uint8, device="cuda")
            sim = ntscsim.FieldSimulator()
            sim.set_mode(mode)
            sim.set_mixed_forms(tuned)
            sim.run_mixed_descs(sets, G.build(sim, descs, src_t, dst_t), w, h)
            assert sim.last_kernels() == (want if tuned else T.generic_names(sets, rt="float"))
            out[(mode, tuned)] = (dst_t, sim.rng_pos)
            sim.sync()
            sim.close()
    ref, end = out[(_capi.MODE_FAST32, False)]
    assert bool((ref != FILL).any())
    for key, (t, pos) in out.items():
        assert pos == end and torch.equal(t, ref), key


# ---------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("own_half", [False, True], ids=["forty_sets", "half_on_the_ctx_set"])
def test_one_set_per_field(own_half):
    """40 fields of 64 x 16 over 40 sets; own_half: every other descriptor takes set -1 on a -vhs context"""
    sets = G.forty_sets()
    descs = [desc(-1 if own_half and i % 2 else i, i % 4, i, i & 1, i) for i in range(40)]
    ctx_flags = ["-vhs"] if own_half else []
    names, _ = T.tuned_vs_oracle(sets, descs, 64, 16, 4, 40, ctx_flags=ctx_flags, warmup=(1, 2) if own_half else None)
    named = [sets[d["set"]] if d["set"] >= 0 else L.make_params(ctx_flags) for d in descs]
    assert names == T.derived_names(named, 64, 16)
    if own_half:
        assert "k_mixed_decode_fast<true,double>" in names


def test_many_descriptors_with_explicit_positions():
    rnd = random.Random(7)
    which = ["default", "vhs", "vhs_ep", "vhs_svideo", "catv", "phase90", "dropout_often", "chroma_noise_only"]
    sets = [L.make_params(FLAGS[n]) for n in which]
    descs = [desc(rnd.randrange(8), i % 4, i, i & 1, i, pos=rnd.randrange(0, 150000)) for i in range(1200)]
    names, _ = T.tuned_vs_oracle(sets, descs, 64, 16, 4, 1200, start=99)
    assert names == T.derived_names(sets, 64, 16)


def test_shared_frames_bob_and_interlaced_sources():
    sets = [L.make_params(["-vhs"]), L.make_params([]), L.make_params(FLAGS["vhs_svideo"])]
    descs = [
        desc(0, 0, 0, 1, 0), desc(1, 0, 0, 0, 1),
        desc(2, 1, 1, 0, 2, bob=True), desc(1, 1, 2, 1, 3),
        desc(0, 2, 3, 1, 4, il=1, tff=1), desc(1, 2, 4, 0, 5, il=1, tff=0),
        desc(0, 3, 5, 1, 6, bob=True, il=1, tff=1), desc(2, 3, 6, 0, 7), desc(-1, 0, 6, 1, 8),
    ]
    for w, h in ((96, 32), (96, 33), (100, 32)):
        names, _ = T.tuned_vs_oracle(sets, descs, w, h, 4, 7, ctx_flags=FLAGS["vhs_ep"], seed=w + h)
        assert names == T.derived_names(sets + [L.make_params(FLAGS["vhs_ep"])], w, h, bob=True)
        assert names[-1] == "k_mixed_bob" and "k_mixed_decode_fast_sv<double>" in names


def test_calls_in_flight_share_the_scratch():
    """Three tuned calls of different sizes and a single-set call on one context and stream, one sync."""
    torch = T.torch_mod()
    w, h = 64, 34
    ctx_params = L.make_params(["-vhs"])
    sets = [L.make_params(FLAGS[n]) for n in ("default", "vhs_svideo", "vhs_ep", "catv")]
    calls = [
        [desc(i % 4, i % 3, i, i & 1, i) for i in range(9)],
        [desc((i * 3) % 4 if i % 5 else -1, i % 3, 9 + i, i & 1, 100 + i) for i in range(30)],
        None,
        [desc(3 - i % 4, i % 3, 45 + i, i & 1, 200 + i) for i in range(4)],
    ]
    single = [desc(-1, i % 3, 39 + i, i & 1, 300 + i) for i in range(6)]
    n_dst = 49
    srcs = [L.noise_frame(w, h, 0x777 + j) for j in range(3)]
    exp = np.full((n_dst, h, w, 4), FILL, np.uint8)
    o, cursor = G.Oracle(), 5
    for c in calls:
        cursor = o.run(G.params_lookup(sets, ctx_params), single if c is None else c, srcs, exp, w, h, cursor)
    src_t = torch.from_numpy(np.stack(srcs)).cuda()
    dst_t = torch.full((n_dst, h, w, 4), FILL, dtype=torch.uint8, device="cuda")
    sim = ntscsim.FieldSimulator(params=ctx_params)
    sim.set_mixed_forms(True)
    sim.rng_pos = 5
    set_arr = sim.build_sets(sets)
    keep, ran = [], []
    for c in calls:
        if c is None:
            keep.append(sim.fields(src_t, dst_t, [(d["src"], d["dst"], d["field"], d["fieldno"]) for d in single]))
        else:
            keep.append(G.build(sim, c, src_t, dst_t))
            sim.run_mixed_descs(set_arr, keep[-1], w, h)
        ran.append(sim.last_kernels())
    assert sim.rng_pos == cursor
    sim.sync()
    got = dst_t.cpu().numpy()
    sim.close()
    bad = [k for k in range(n_dst) if not np.array_equal(got[k], exp[k])]
    assert not bad, bad
    assert all(any("k_mixed_decode_fast" in k for k in r) for r in (ran[0], ran[1], ran[3])), ran
    assert not any("mixed" in k for k in ran[2]), ran


def test_profiling_covers_a_tuned_call():
    torch = T.torch_mod()
    w, h = 96, 32
    sets, descs = family_sets()
    src_t = torch.from_numpy(np.stack([L.noise_frame(w, h, 0x2345678 + j) for j in range(4)])).cuda()
    dst_t = torch.full((len(descs), h, w, 4), FILL, dtype=torch.uint8, device="cuda")
    sim = ntscsim.FieldSimulator()
    sim.set_mixed_forms(True)
    sim.set_profiling(True)
    for _ in range(2):
        sim.run_mixed_descs(sets, G.build(sim, descs, src_t, dst_t), w, h)
    sim.sync()
    t = sim.timings_ms()
    sim.close()
    assert t["calls"] == 2
    assert all(np.isfinite(t[k]) and t[k] > 0 for k in ("setup", "encode", "decode", "total")), t
    assert t["setup"] + t["encode"] + t["decode"] <= t["total"] * 1.001


# ---------------------------------------------------------------------------------------------- 8
def test_refusals_are_unchanged_under_tuned():
    """The table of tests/test_mixed_fields_gpu.py's refusal test, with the switch on: same codes, nothing enqueued, the
    position where it was -- and the next call is exact."""
    torch = T.torch_mod()
    w, h = 96, 32
    srcs = [L.noise_frame(w, h, 5 + j) for j in range(2)]
    src_t = torch.from_numpy(np.stack(srcs)).cuda()
    dst_t = torch.full((4, h, w, 4), FILL, dtype=torch.uint8, device="cuda")
    sim = ntscsim.FieldSimulator(["-vhs"])
    sim.set_mixed_forms(True)
    sim.rng_pos = 1234
    lib, hnd = sim._lib, sim._h
    good = [L.make_params([]), L.make_params(["-vhs"])]

    def call(sets, descs, n_sets=None, w_=w, h_=h, null_descs=False, edit=None):
        arr = G.build(sim, descs, src_t, dst_t)
        if edit:
            edit(arr)
        sa = sim.build_sets(sets) if sets else None
        ns = (0 if sa is None else len(sa)) if n_sets is None else n_sets
        rc = lib.ntscsim_mixed_fields_device(hnd, sa, ns, None if null_descs else arr, len(arr), w_, h_, None)
        sim.sync()
        return rc

    two = [desc(0, 0, 0, 1, 0), desc(1, 1, 1, 0, 1)]
    bad_size = L.make_params([])
    bad_size.struct_size = 12
    neg_noise = L.make_params([], video_noise=-1)
    ghost = L.make_params(["-vhs"], ghost_taps=1)
    ghost.ghost_delay[0], ghost.ghost_gain[0] = 8, 64

    def null_src(arr):
        arr[1].d.src_dev = None

    def null_dst(arr):
        arr[0].d.dst_dev = None

    def short_row(arr):
        arr[1].d.dst_linesize = 4 * w - 4

    refused = [
        ("set past the table", call(good, [desc(0, 0, 0, 1, 0), desc(2, 1, 1, 0, 1)]), _capi.E_ARG),
        ("set below -1", call(good, [desc(-2, 0, 0, 1, 0)]), _capi.E_ARG),
        ("n_sets < 0", call(good, two, n_sets=-1), _capi.E_ARG),
        ("NULL sets that should hold something", call(None, two, n_sets=2), _capi.E_ARG),
        ("wrong struct_size", call([good[0], bad_size], two), _capi.E_ARG),
        ("invalid params", call([good[0], neg_noise], two), _capi.E_PARAM),
        ("ghost taps", call([good[0], ghost], two), _capi.E_PARAM),
        ("shared destination, equal parity", call(good, [desc(0, 0, 2, 1, 0), desc(1, 1, 2, 1, 1)]), _capi.E_ARG),
        ("bob shares a frame", call(good, [desc(0, 0, 2, 1, 0, bob=True), desc(1, 1, 2, 0, 1)]), _capi.E_ARG),
        ("NULL source", call(good, two, edit=null_src), _capi.E_ARG),
        ("NULL destination", call(good, two, edit=null_dst), _capi.E_ARG),
        ("NULL descriptors", call(good, two, null_descs=True), _capi.E_ARG),
        ("field 2", call(good, [desc(0, 0, 0, 2, 0)]), _capi.E_ARG),
        ("width below 16", call(good, two, w_=8), _capi.E_SIZE),
        ("linesize below 4 * width", call(good, two, edit=short_row), _capi.E_SIZE),
    ]
    assert [(n, rc) for n, rc, want in refused if rc != want] == []
    assert sim.rng_pos == 1234
    assert bool((dst_t == FILL).all()), "a refused call wrote to a destination"
    assert lib.ntscsim_mixed_fields_device(hnd, None, 0, None, 0, w, h, None) == _capi.OK
    assert sim.rng_pos == 1234
    # the next call is exact
    assert call([good[0], good[1], bad_size, neg_noise, ghost], two) == _capi.OK
    assert sim.last_kernels() == ["k_mixed_setup", "k_mixed_encode_fast<double>", "k_mixed_decode_fast<false,double>",
                                  "k_mixed_decode_fast<true,double>"]
    exp = np.full((4, h, w, 4), FILL, np.uint8)
    end = G.Oracle().run(G.params_lookup(good, None), two, srcs, exp, w, h, 1234)
    assert sim.rng_pos == end
    assert np.array_equal(dst_t.cpu().numpy(), exp)
    sim.close()
