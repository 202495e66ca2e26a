"""ntscsim_mixed_fields_device on the GPU: fields of one call that name different parameter sets, one launch of each
kernel.  Every comparison is byte for byte over whole destination buffers -- untouched rows and row padding included --
and the yardstick is the CPU oracle, never the product: for each descriptor the oracle runs with the parameters of the
descriptor's set from the descriptor's rand() position (ntsc_oracle_bob where the descriptor asks for bob).

A descriptor of these tests is a dict: set, src (frame index), dst (frame index), field, fieldno, and optionally il, tff,
bob, pos (an explicit rand() position; None = NTSCSIM_RNG_AUTO)."""
import ctypes as C
import random

import numpy as np
import pytest

import _libs as L
import cases
import ntscsim
from ntscsim import _capi

pytestmark = pytest.mark.gpu

FILL = 0x5A
FLAGS = {c[0]: c[1] for c in cases.CASES}


def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def desc(set_, src, dst, field, fieldno, il=0, tff=0, bob=False, pos=None):
    return dict(set=set_, src=src, dst=dst, field=field, fieldno=fieldno, il=il, tff=tff, bob=bob, pos=pos)


class Oracle:
    """One rand() stream moved to where each descriptor starts; the parameters change per descriptor."""

    def __init__(self):
        self.o = L.OracleStream(None)

    def at(self, pos):
        if pos < self.o.rng_pos:
            self.o = L.OracleStream(None)
        self.o.skip(pos - self.o.rng_pos)

    def run(self, params_of, descs, srcs, exp, w, h, start):
        """exp: [n_dst, h, w, 4], updated in place; returns the position behind the last descriptor"""
        cursor = start
        for d in descs:
            p = params_of(d["set"])
            if d["pos"] is not None:
                cursor = d["pos"]
            self.at(cursor)
            self.o.p = p
            self.o.field(exp[d["dst"]], srcs[d["src"]], d["field"], d["fieldno"], d["il"], d["tff"])
            if d["bob"]:
                L.oracle().ntsc_oracle_bob(L._ptr(exp[d["dst"]]), w * 4, w, h, d["field"])
            cursor += ntscsim.calls_per_field(p, w, h, d["field"])
            assert self.o.rng_pos == cursor
        return cursor


def params_lookup(sets, ctx_params):
    return lambda s: ctx_params if s < 0 else sets[s]


def build(sim, descs, src_t, dst_t):
    jobs = [(d["src"], d["dst"], d["field"], d["fieldno"]) for d in descs]
    return sim.build_mixed_descs([d["set"] for d in descs], src_t, dst_t, jobs, bob=[d["bob"] for d in descs],
                                 interlaced=[d["il"] for d in descs], tff=[d["tff"] for d in descs],
                                 rng_pos=[_capi.RNG_AUTO if d["pos"] is None else d["pos"] for d in descs])


def mixed_vs_oracle(sets, descs, w, h, n_src, n_dst, ctx_flags=(), start=0, pad=0, seed=0, warmup=None):
    """One mixed call against the oracle.  pad: extra pixels per row of the source and destination buffers (linesizes
    that are no multiple of 16; the padding is compared too).  Returns (last_kernels, rng_pos after)."""
    torch = torch_mod()
    ctx_params = L.make_params(list(ctx_flags))
    srcs = [L.noise_frame(w, h, 0x2345678 + seed + j) for j in range(n_src)]
    exp = np.full((n_dst, h, w, 4), FILL, np.uint8)
    end = Oracle().run(params_lookup(sets, ctx_params), descs, srcs, exp, w, h, start)
    src_pad = np.full((n_src, h, w + pad, 4), 0xC3, np.uint8)
    src_pad[:, :, :w] = np.stack(srcs)
    src_t = torch.from_numpy(src_pad).cuda()
    dst_t = torch.full((n_dst, h, w + pad, 4), FILL, dtype=torch.uint8, device="cuda")
    sim = ntscsim.FieldSimulator(params=ctx_params)
    sim.rng_pos = start
    if warmup:
        sim.debug_set_warmup(*warmup)        # (a shorter look-back of the row-start states: the walk behind it is exact)
    arr = build(sim, descs, src_t[:, :, :w], dst_t[:, :, :w])
    sim.run_mixed_descs(list(sets), arr, w, h)
    names, pos = sim.last_kernels(), sim.rng_pos
    sim.sync()
    got = dst_t.cpu().numpy()
    sim.close()
    assert pos == end
    bad = [k for k in range(n_dst) if not np.array_equal(got[k, :, :w], exp[k])]
    assert not bad, "destination frames %r differ from the oracle" % bad[:10]
    if pad:
        assert (got[:, :, w:] == FILL).all(), "row padding was written"
    return names, pos


# ---------------------------------------------------------------------------------------------- 1
FAMILY = ["default", "vhs", "vhs_ep", "vhs_lp_only", "vhs_svideo", "vhs_noblend", "vhs_pal", "vhs_full_outlp", "no_outlp",
          "no_inlp", "catv", "catv4_vhs", "phase90", "phase270", "nocolor_vhs", "amp30", "dropout_often", "phase_noise20",
          "chroma_noise_only", "noise0", "hs_neg", "hs_pos", "hs_nonoise"]


def family_call():
    sets = [L.make_params(FLAGS[n]) for n in FAMILY]
    n = len(sets)
    # two fields per set, the sets interleaved: no two neighbours share one
    descs = [desc(s, (rep * n + s) % 4, rep * n + s, (s + rep) & 1, 10 * s + rep) for rep in range(2) for s in range(n)]
    return sets, descs


def test_every_switch_family_in_one_call():
    sets, descs = family_call()
    names, _ = mixed_vs_oracle(sets, descs, 96, 32, 4, len(descs))
    assert names == ["k_mixed_setup", "k_mixed_encode<double>", "k_mixed_decode<false,false,double>",
                     "k_mixed_decode<true,true,double>", "k_mixed_decode<true,false,double>"]


def test_every_switch_family_fast32_equals_the_generic_single_set_kernels():
    """FAST32: the same kernels with float filter states.  One single-set context per set with the generic kernels forced
    runs the same arithmetic, so the bytes are equal."""
    torch = torch_mod()
    w, h = 96, 32
    sets, descs = family_call()
    srcs = np.stack([L.noise_frame(w, h, 0x2345678 + j) for j in range(4)])
    src_t = torch.from_numpy(srcs).cuda()
    dst_t = torch.full((len(descs), h, w, 4), FILL, dtype=torch.uint8, device="cuda")
    ref_t = torch.full((len(descs), h, w, 4), FILL, dtype=torch.uint8, device="cuda")
    sim = ntscsim.FieldSimulator()
    sim.set_mode(_capi.MODE_FAST32)
    sim.run_mixed_descs(sets, build(sim, descs, src_t, dst_t), w, h)
    assert sim.last_kernels() == ["k_mixed_setup", "k_mixed_encode<float>", "k_mixed_decode<false,false,float>",
                                  "k_mixed_decode<true,true,float>", "k_mixed_decode<true,false,float>"]
    end = sim.rng_pos
    sim.sync()
    singles = []
    for s, p in enumerate(sets):
        one = ntscsim.FieldSimulator(params=p)
        one.set_mode(_capi.MODE_FAST32)
        one.debug_force_generic(True)
        singles.append(one)
    cursor = 0
    for d in descs:
        one = singles[d["set"]]
        one.rng_pos = cursor
        one.fields(src_t, ref_t, [(d["src"], d["dst"], d["field"], d["fieldno"])])
        assert all("fast" not in k and "pipe" not in k for k in one.last_kernels()), one.last_kernels()
        cursor = one.rng_pos
    for one in singles:
        one.sync()
    assert cursor == end
    assert torch.equal(dst_t, ref_t)
    assert (dst_t != FILL).any()
    for one in singles:
        one.close()
    sim.close()


# ---------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("h", [125, 126, 127, 128, 129, 130, 33])
def test_block_edges(h):
    """Lslot on both sides of 63 and 64 (and an odd height); groups of 1, 2 and 3 fields, so group row counts land on,
    one short of and one past multiples of 63 and 64; the groups in both orders.  -vhs blends chroma vertically: a wrong
    halo at a group's first decoder block shows in its row 0 or 63."""
    sets = [L.make_params(["-vhs"]), L.make_params(FLAGS["vhs_noblend"]), L.make_params([])]
    for order in ([0, 1, 2], [2, 1, 0]):
        descs = []
        for s in order:
            for k in range(s + 1):
                descs.append(desc(s, len(descs) % 3, len(descs), (k + s) & 1, 7 * s + k))
        mixed_vs_oracle(sets, descs, 64, h, 3, len(descs), seed=h)


# ---------------------------------------------------------------------------------------------- 3
def forty_sets():
    rnd = random.Random(20240607)
    sets = []
    for i in range(40):
        flags = ["-vhs"] if i % 3 else []
        flags += ["-noise", str(rnd.randrange(0, 60)), "-chroma-noise", str(rnd.randrange(0, 50)),
                  "-chroma-phase-noise", str(rnd.randrange(0, 12))]
        if i % 3 == 2:
            flags += ["-vhs-svideo", "1"]
        sets.append(L.make_params(flags, vhs_out_sharpen=0.25 * rnd.randrange(0, 12),
                                  vhs_head_switching_point=rnd.uniform(0.02, 0.2) if i % 2 else 1.0 - 4.5 / 262.5 * rnd.random()))
    return sets


@pytest.mark.parametrize("own_half", [False, True], ids=["forty_sets", "half_on_the_ctx_set"])
def test_one_set_per_field(own_half):
    """40 fields of 64 x 16, 40 sets: 8 rows per group, so most lanes of every block are idle.  own_half: every other
    descriptor takes set -1 on a context created with -vhs, and ntscsim_debug_set_warmup shortens the look-back."""
    sets = forty_sets()
    descs = [desc(-1 if own_half and i % 2 else i, i % 4, i, i & 1, i) for i in range(40)]
    names, _ = mixed_vs_oracle(sets, descs, 64, 16, 4, 40, ctx_flags=["-vhs"] if own_half else [],
                               warmup=(1, 2) if own_half else None)
    assert names[0] == "k_mixed_setup" and names[1] == "k_mixed_encode<double>" and len(names) == 5


# ---------------------------------------------------------------------------------------------- 4
def test_many_descriptors_with_explicit_positions():
    """1,200 fields over 8 sets, every one at a position of its own, not monotonic; the context ends behind the last."""
    rnd = random.Random(7)
    names = ["default", "vhs", "vhs_ep", "vhs_svideo", "catv", "phase90", "dropout_often", "chroma_noise_only"]
    sets = [L.make_params(FLAGS[n]) for n in names]
    descs = [desc(rnd.randrange(8), i % 4, i, i & 1, i, pos=rnd.randrange(0, 150000)) for i in range(1200)]
    _, pos = mixed_vs_oracle(sets, descs, 64, 16, 4, 1200, start=99)
    last = descs[-1]
    assert pos == last["pos"] + ntscsim.calls_per_field(sets[last["set"]], 64, 16, last["field"])


# ---------------------------------------------------------------------------------------------- 5
def test_shared_frames_bob_interlaced_sources_and_unaligned_rows():
    sets = [L.make_params(["-vhs"]), L.make_params([]), L.make_params(FLAGS["vhs_svideo"])]
    descs = [
        desc(0, 0, 0, 1, 0), desc(1, 0, 0, 0, 1),                          # the two fields of frame 0, two sets
        desc(2, 1, 1, 0, 2, bob=True), desc(1, 1, 2, 1, 3),                # bob among plain ones
        desc(0, 2, 3, 1, 4, il=1, tff=1), desc(1, 2, 4, 0, 5, il=1, tff=0),  # interlaced sources, tff and bff
        desc(0, 3, 5, 1, 6, bob=True, il=1, tff=1), desc(2, 3, 6, 0, 7), desc(-1, 0, 6, 1, 8),
    ]
    for w, h, pad in ((96, 32, 1), (96, 33, 3), (100, 32, 0)):
        names, _ = mixed_vs_oracle(sets, descs, w, h, 4, 7, ctx_flags=FLAGS["vhs_ep"], pad=pad, seed=w + h)
        assert names[-1] == "k_mixed_bob" and len(names) == 6


# ---------------------------------------------------------------------------------------------- 6
def test_calls_in_flight_share_the_scratch():
    """Three mixed calls of different sizes and a single-set call on one context and stream, back to back: each reuses
    the scratch and the record buffers of the one before.  One sync, then everything is compared."""
    torch = torch_mod()
    w, h = 64, 34
    ctx_params = L.make_params(["-vhs"])
    sets = [L.make_params(FLAGS[n]) for n in ("default", "vhs_svideo", "vhs_ep", "catv")]
    calls = [
        [desc(i % 4, i % 3, i, i & 1, i) for i in range(9)],
        [desc((i * 3) % 4 if i % 5 else -1, i % 3, 9 + i, i & 1, 100 + i) for i in range(30)],
        None,                                                              # the single-set call: 6 fields of the ctx's set
        [desc(3 - i % 4, i % 3, 45 + i, i & 1, 200 + i) for i in range(4)],
    ]
    single = [desc(-1, i % 3, 39 + i, i & 1, 300 + i) for i in range(6)]
    n_dst = 49
    srcs = [L.noise_frame(w, h, 0x777 + j) for j in range(3)]
    exp = np.full((n_dst, h, w, 4), FILL, np.uint8)
    o, cursor = Oracle(), 5
    for c in calls:
        cursor = o.run(params_lookup(sets, ctx_params), single if c is None else c, srcs, exp, w, h, cursor)
    src_t = torch.from_numpy(np.stack(srcs)).cuda()
    dst_t = torch.full((n_dst, h, w, 4), FILL, dtype=torch.uint8, device="cuda")
    sim = ntscsim.FieldSimulator(params=ctx_params)
    sim.rng_pos = 5
    set_arr = sim.build_sets(sets)
    keep = []
    for c in calls:
        if c is None:
            keep.append(sim.fields(src_t, dst_t, [(d["src"], d["dst"], d["field"], d["fieldno"]) for d in single]))
        else:
            keep.append(build(sim, c, src_t, dst_t))
            sim.run_mixed_descs(set_arr, keep[-1], w, h)
    assert sim.rng_pos == cursor
    sim.sync()
    got = dst_t.cpu().numpy()
    sim.close()
    bad = [k for k in range(n_dst) if not np.array_equal(got[k], exp[k])]
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- 7
def test_refusals_write_nothing_and_leave_the_position():
    torch = torch_mod()
    w, h = 96, 32
    src_t = torch.from_numpy(np.stack([L.noise_frame(w, h, 5 + j) for j in range(2)])).cuda()
    dst_t = torch.full((4, h, w, 4), FILL, dtype=torch.uint8, device="cuda")
    sim = ntscsim.FieldSimulator(["-vhs"])
    sim.rng_pos = 1234
    lib, hnd = sim._lib, sim._h
    good = [L.make_params([]), L.make_params(["-vhs"])]

    def call(sets, descs, n_sets=None, w_=w, h_=h, null_descs=False, edit=None):
        arr = build(sim, descs, src_t, dst_t)
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
    assert lib.ntscsim_params_validate(C.byref(ghost)) == _capi.OK        # (a set the single-set calls accept)

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
    # n == 0 succeeds and does nothing; a set nobody names is not looked at
    assert lib.ntscsim_mixed_fields_device(hnd, None, 0, None, 0, w, h, None) == _capi.OK
    assert sim.rng_pos == 1234
    assert call([good[0], good[1], bad_size, neg_noise, ghost], two) == _capi.OK
    assert sim.rng_pos == 1234 + ntscsim.calls_per_field(good[0], w, h, 1) + ntscsim.calls_per_field(good[1], w, h, 0)
    assert bool((dst_t[:2] != FILL).any()) and bool((dst_t[2:] == FILL).all())
    sim.close()


# ---------------------------------------------------------------------------------------------- 8
def test_the_single_set_call_keeps_its_kernels_after_a_mixed_call():
    torch = torch_mod()
    w, h, n = 96, 32, 4
    p = L.make_params(["-vhs"])
    frames = [L.noise_frame(w, h, 0x1234567 + i) for i in range(n // 2)]
    jobs = [(k // 2, k, (k & 1) ^ 1, k) for k in range(n)]
    src_t = torch.from_numpy(np.stack(frames)).cuda()

    fresh = ntscsim.FieldSimulator(params=p)
    d0 = torch.zeros((n, h, w, 4), dtype=torch.uint8, device="cuda")
    fresh.fields(src_t, d0, jobs)
    today = fresh.last_kernels()
    fresh.sync()
    fresh.close()
    assert "k_encode_fast<double>" in today and "k_decode_fast<true,double>" in today, today

    sim = ntscsim.FieldSimulator(params=p)
    sets, descs = family_call()
    scratch_t = torch.zeros((len(descs), h, w, 4), dtype=torch.uint8, device="cuda")
    src4 = torch.from_numpy(np.stack([L.noise_frame(w, h, 0x2345678 + j) for j in range(4)])).cuda()
    sim.run_mixed_descs(sets, build(sim, descs, src4, scratch_t), w, h)
    assert sim.last_kernels()[0] == "k_mixed_setup"
    start = sim.rng_pos
    dst_t = torch.zeros((n, h, w, 4), dtype=torch.uint8, device="cuda")
    sim.fields(src_t, dst_t, jobs)
    assert sim.last_kernels() == today
    sim.sync()
    got = dst_t.cpu().numpy()
    sim.close()
    exp = np.zeros((n, h, w, 4), np.uint8)
    o = L.OracleStream(p)
    o.skip(start)
    for (si, di, field, fieldno) in jobs:
        o.field(exp[di], frames[si], field, fieldno)
    assert np.array_equal(got, exp)


# ---------------------------------------------------------------------------------------------- 9
def _many_sets(n, first_level):
    """n sets that differ in noise levels and each have a chroma phase-noise level of their own (a cos/sin table each)"""
    return [L.make_params(["-vhs"] if i % 2 else [], video_noise=i % 7, video_chroma_noise=(i * 5) % 11,
                          video_chroma_phase_noise=first_level + i) for i in range(n)]


def test_more_sets_than_the_table_cache_holds_in_flight():
    """300 sets in a call, back to back with no synchronisation, on the contexts' table caches of 256 entries each.
    Sets that differ in noise LEVELS share their tables (at most 16 draw layouts a geometry), so calls of 300 such sets
    never drop the caches; 300 phase-noise levels need 300 cos/sin tables: the call that brings them past the bound drops
    the caches once, and the same call again finds all of them.  Every call's bytes are the oracle's."""
    torch = torch_mod()
    w, h, n = 64, 16, 300
    levels = [L.make_params(["-vhs"] if i % 3 else [], video_noise=i % 13, video_chroma_noise=(i * 7) % 17,
                            video_chroma_phase_noise=i % 5) for i in range(n)]
    calls = [(levels, 0), (levels, 0), (_many_sets(n, 1), 1), (_many_sets(n, 301), 2), (_many_sets(n, 301), 2)]
    ctx_params = L.make_params([])
    srcs = [L.noise_frame(w, h, 0x4242 + j) for j in range(4)]
    src_t = torch.from_numpy(np.stack(srcs)).cuda()
    dst_t = torch.full((len(calls) * n, h, w, 4), FILL, dtype=torch.uint8, device="cuda")
    exp = np.full((len(calls) * n, h, w, 4), FILL, np.uint8)
    sim = ntscsim.FieldSimulator(params=ctx_params)
    o, cursor, keep, stats = Oracle(), 0, [], []
    for k, (sets, _) in enumerate(calls):
        descs = [desc(i, i % 4, k * n + i, i & 1, i) for i in range(n)]
        cursor = o.run(params_lookup(sets, ctx_params), descs, srcs, exp, w, h, cursor)
        keep.append((sim.build_sets(sets), build(sim, descs, src_t, dst_t)))
    for sa, arr in keep:                                   # (everything is enqueued before anything is waited for)
        sim.run_mixed_descs(sa, arr, w, h)
        stats.append(sim.debug_mixed_tables())
    assert sim.rng_pos == cursor
    sim.sync()
    got = dst_t.cpu().numpy()
    sim.close()
    # levels 0..4: 4 tables, no drop, twice; +300 levels: past 256, dropped once and rebuilt; 300 other levels: dropped
    # again; the same 300 again: all cached
    assert [s[2] for s in stats] == [0, 0, 1, 2, 2], stats
    assert stats[0] == stats[1] and stats[0][1] == 4 and stats[0][0] <= 16
    assert stats[3] == stats[4] and stats[4][1] == 300
    bad = [k for k in range(len(exp)) if not np.array_equal(got[k], exp[k])]
    assert not bad, bad[:10]


# ---------------------------------------------------------------------------------------------- 10
def test_float_mode_runs_the_fast32_forms_and_profiling_covers_the_call():
    torch = torch_mod()
    w, h = 96, 32
    sets, descs = family_call()
    src_t = torch.from_numpy(np.stack([L.noise_frame(w, h, 0x2345678 + j) for j in range(4)])).cuda()
    out = {}
    for mode in (_capi.MODE_FAST32, _capi.MODE_FLOAT):
        dst_t = torch.full((len(descs), h, w, 4), FILL, dtype=torch.uint8, device="cuda")
        sim = ntscsim.FieldSimulator()
        sim.set_mode(mode)
        sim.set_profiling(True)
        sim.run_mixed_descs(sets, build(sim, descs, src_t, dst_t), w, h)
        assert sim.last_kernels() == ["k_mixed_setup", "k_mixed_encode<float>", "k_mixed_decode<false,false,float>",
                                      "k_mixed_decode<true,true,float>", "k_mixed_decode<true,false,float>"]
        sim.sync()
        t = sim.timings_ms()
        assert t["calls"] == 1 and t["total"] > 0 and t["setup"] > 0 and t["encode"] > 0 and t["decode"] > 0, t
        assert t["setup"] + t["encode"] + t["decode"] <= t["total"] * 1.001
        out[mode] = dst_t
        sim.close()
    assert torch.equal(out[_capi.MODE_FAST32], out[_capi.MODE_FLOAT])
    assert bool((out[_capi.MODE_FLOAT] != FILL).any())
