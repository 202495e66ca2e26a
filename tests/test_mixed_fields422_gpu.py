"""ntscsim_mixed_fields422_device on the GPU: YUV422P fields of one call that name different parameter sets, one launch of
each kernel.  The yardstick is the CPU oracle, never the product: TocompOracleStream(params, OOB_MEMORY) with
tocomp_oracle_render_field / tocomp_oracle_black_key, run descriptor by descriptor in the caller's order, each with the
parameters of its set and from its own rand() position.  Frames are single buffers with planes as views, and WHOLE
buffers are compared -- destination, feedback and source frames, untouched rows, row padding and the slack behind the
planes included.  Rows are padded by 32 unless a test says otherwise, so no byte is excluded; the one tight-row test
excludes what tests/test_variant422.py excludes: the right margin of the frame's last row.

A descriptor of these tests is a dict: set, dst (an L.Yuv422), field, fieldno, and optionally src (an L.Yuv422 whose
height is the source height), flt (an L.Yuv422), flags (F422_*), pos (an explicit rand() position; None = AUTO)."""
import ctypes as C

import numpy as np
import pytest

import _libs as L
import cases422
import ntscsim
from ntscsim import _capi

pytestmark = pytest.mark.gpu

MARGIN_Y, MARGIN_C = 24, 14          # the constants of tests/test_variant422.py
PAD = 32
NAMES_ALL = ["k_mixed_setup", "k422_mixed_render", "k422_mixed_bkey", "k422_mixed_halo", "k422_mixed_process"]


def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def calls422(p, w, h, field):
    return int(L.product().ntscsim_rng_calls_per_field_422(C.byref(p), w, h, field))


def desc(set_, dst, field, fieldno, src=None, flt=None, flags=0, pos=None):
    return dict(set=set_, dst=dst, field=field, fieldno=fieldno, src=src, flt=flt, flags=flags, pos=pos)


def oracle_run(params_of, descs, w, h, start):
    """Runs the descriptors on their host frames, in place and in order; returns the position behind the last one."""
    cursor = start
    for d in descs:
        p = params_of(d["set"])
        fl = d["flags"]
        if d["pos"] is not None:
            cursor = d["pos"]
        if d["src"] is not None:
            L.tocomp_oracle_render_field(d["dst"], d["src"], int(bool(fl & _capi.F422_SRC420)),
                                         int(bool(fl & _capi.F422_INTERLACED)), int(bool(fl & _capi.F422_TFF)),
                                         int(bool(fl & _capi.F422_SECOND)), d["field"])
        if d["flt"] is not None and p.black_key_level_feedback >= 0:
            L.tocomp_oracle_black_key(d["dst"], d["flt"], d["field"], p.black_key_level_feedback)
        if not (fl & _capi.F422_NOCOMP):
            o = L.TocompOracleStream(p, L.OOB_MEMORY)
            o.skip(cursor)
            o.process(d["dst"], d["field"], d["fieldno"])
            assert o.rng_pos - cursor == calls422(p, w, h, d["field"])
            cursor = o.rng_pos
    return cursor


def last_row_margin_mask(frame):
    """True where the product must equal the reference on a frame whose luma rows are tighter than W + 2: everything
    but the right margin of the LAST row (tests/test_variant422.py)."""
    m = np.ones(frame.buf.shape, bool)
    for i, marg in ((0, MARGIN_Y), (1, MARGIN_C), (2, MARGIN_C)):
        n = frame.ls[i] * frame.h
        pm = m[frame.off[i]:frame.off[i] + n].reshape(frame.h, frame.ls[i])
        width = frame.w if i == 0 else frame.w // 2
        pm[frame.h - 1, max(0, width - marg):width] = False
    return m


class Call:
    """One mixed call: the frames go to the device as they are, THEN the oracle runs on the host copies."""

    def __init__(self, sets, descs, w, h, ctx_params, start=0):
        torch = torch_mod()
        self.sets, self.descs, self.w, self.h, self.start = list(sets), descs, w, h, start
        self.frames, self.dev = [], {}
        for d in descs:
            for fr in (d["dst"], d["src"], d["flt"]):
                if fr is not None and id(fr) not in self.dev:
                    whole = torch.from_numpy(fr.buf.copy()).cuda()
                    views = [whole[fr.off[i]:fr.off[i] + fr.ls[i] * fr.h].view(fr.h, fr.ls[i]) for i in range(3)]
                    self.dev[id(fr)] = (whole, views)
                    self.frames.append(fr)
        self.before = [fr.buf.copy() for fr in self.frames]
        self.end = oracle_run(lambda s: ctx_params if s < 0 else self.sets[s], descs, w, h, start)

    def jobs(self):
        out = []
        for d in self.descs:
            j = {"dst": self.dev[id(d["dst"])][1], "field": d["field"], "fieldno": d["fieldno"], "flags": d["flags"],
                 "rng_pos": d["pos"]}
            if d["src"] is not None:
                j["src"], j["src_height"] = self.dev[id(d["src"])][1], d["src"].h
            if d["flt"] is not None:
                j["flt"] = self.dev[id(d["flt"])][1]
            out.append(j)
        return out

    def array(self, sim):
        return sim.build_mixed_descs422([d["set"] for d in self.descs], self.jobs())

    def enqueue(self, sim):
        sim.run_mixed_descs422(self.sets, self.array(sim), self.w, self.h)

    def got(self, fr):
        return self.dev[id(fr)][0].cpu().numpy()

    def check(self, masks=None):
        """after a sync: every frame of the call against the oracle's"""
        bad = []
        for k, fr in enumerate(self.frames):
            diff = self.got(fr) != fr.buf
            if masks is not None and id(fr) in masks:
                diff &= masks[id(fr)]
            if diff.any():
                bad.append((k, int(diff.sum()), int(np.argmax(diff))))
        assert not bad, "frames (index, bytes, first) that differ from the oracle: %r" % bad[:10]

    def check_untouched(self):
        for fr, b in zip(self.frames, self.before):
            assert np.array_equal(self.got(fr), b)


def mixed_vs_oracle(sets, descs, w, h, ctx_flags=(), start=0):
    """One mixed call on a fresh ctx against the oracle.  Returns last_kernels()."""
    ctx_params = L.make_params_tocomp(list(ctx_flags))
    call = Call(sets, descs, w, h, ctx_params, start)
    sim = ntscsim.FieldSimulator(params=ctx_params)
    sim.rng_pos = start
    call.enqueue(sim)
    names, pos = sim.last_kernels(), sim.rng_pos
    sim.sync()
    try:
        assert pos == call.end
        call.check()
    finally:
        sim.close()
    return names


def fill_frame(w, h, seed, pad=PAD):
    """a destination frame whose every byte -- padding and slack too -- is pseudo-random"""
    fr = L.Yuv422(w, h, pad)
    fr.buf[:] = np.random.RandomState(seed).randint(0, 256, size=fr.buf.shape, dtype=np.uint8)
    return fr


def noise_frame(w, h, seed, pad=PAD):
    """a frame of video levels in pseudo-random padding"""
    fr = fill_frame(w, h, seed ^ 0x5555, pad)
    src = L.yuv_noise(w, h, seed)
    for i in range(3):
        fr.pix(i)[:] = src.pix(i)
    return fr


# ---------------------------------------------------------------------------------------------- 1
def test_every_switch_family_in_one_call():
    """The flag sets of all of cases422.CASES422 (each distinct flag list is one set) at 96x32, every case with two fields
    on frames of their own rendered from its own kind of source, the descriptors ordered so that no two neighbours name
    one set.  Five cases run plain -vhs: that group fills three workgroups, so the halo kernel runs too."""
    w, h = 96, 32
    flag_lists = []
    for c in cases422.CASES422:
        if c[1] not in flag_lists:
            flag_lists.append(c[1])
    sets = [L.make_params_tocomp(f) for f in flag_lists]
    todo = []
    for rep in range(2):
        for ci, c in enumerate(cases422.CASES422):
            src = cases422.make_source422(c[5], w, h, 2 * ci + rep, PAD)
            todo.append(desc(flag_lists.index(c[1]), fill_frame(w, h, 900 + 2 * ci + rep), (rep & 1) ^ 1, 2 * ci + rep, src=src))
    descs = []
    while todo:          # of the descriptors that name another set than the one before: the first of the set with most to go
        left = [sum(1 for d in todo if d["set"] == s) for s in range(len(sets))]
        ok = [i for i, d in enumerate(todo) if not descs or d["set"] != descs[-1]["set"]]
        descs.append(todo.pop(max(ok, key=lambda i: (left[todo[i]["set"]], -i))))
    assert all(a["set"] != b["set"] for a, b in zip(descs, descs[1:])) and len(descs) == 2 * len(cases422.CASES422)
    names = mixed_vs_oracle(sets, descs, w, h, start=11)
    assert names == ["k_mixed_setup", "k422_mixed_render", "k422_mixed_halo", "k422_mixed_process"]


# ---------------------------------------------------------------------------------------------- 2
EDGE_FLAGS = [["-vhs"], ["-vhs", "-vhs-chroma-vblend", "0"], []]


@pytest.mark.parametrize("order", ["first_use_012", "first_use_210"])
@pytest.mark.parametrize("rot", [0, 1, 2])
@pytest.mark.parametrize("h", [125, 126, 127, 128, 129, 130, 33])
def test_block_edges(h, rot, order):
    """Lslot on both sides of 63 and 64 (and one odd height, one small): groups of 1, 2 and 3 fields, every set with every
    group size (rot), in both group orders.  A wrong halo row, or one taken across a group edge, shows in row 0 or 63 of
    a group through the vertical blend of the VCR's chroma."""
    w = 64
    sets = [L.make_params_tocomp(f) for f in EDGE_FLAGS]
    size_of = {s: 1 + (s + rot) % 3 for s in range(3)}
    descs, k = [], 0
    # interleaved: set 0, 1, 2, then those that still have fields to go
    for rnd in range(3):
        for s in range(3):
            if rnd < size_of[s]:
                descs.append(desc(s, noise_frame(w, h, 40 * h + k), (k & 1) ^ 1, k))
                k += 1
    if order == "first_use_210":
        descs.reverse()
    names = mixed_vs_oracle(sets, descs, w, h, start=5)
    halo = 3 * ((h + 1) // 2) > 63        # the group of three fields fills more than one workgroup of 63 rows
    assert names == ["k_mixed_setup"] + (["k422_mixed_halo"] if halo else []) + ["k422_mixed_process"]


# ---------------------------------------------------------------------------------------------- 3
def test_tight_rows():
    """linesize == width: the separator's two bytes past a row are the next row's first pixels (the OTHER field's, which
    this call does not write) and, behind the last row, outside the luma plane: the documented exclusion.  The same
    descriptors on rows padded by 2 bytes pass with nothing excluded."""
    w, h = 64, 34
    sets = [L.make_params_tocomp(f) for f in (["-vhs"], [], ["-vhs", "-vhs-svideo", "1", "-vhs-speed", "lp"])]
    for pad in (0, 2):
        descs = [desc(k % 3, noise_frame(w, h, 70 + k, pad), (k & 1) ^ 1, k) for k in range(7)]
        ctx_params = L.make_params_tocomp([])
        call = Call(sets, descs, w, h, ctx_params)
        sim = ntscsim.FieldSimulator(params=ctx_params)
        call.enqueue(sim)
        pos = sim.rng_pos
        sim.sync()
        sim.close()
        assert pos == call.end
        call.check({id(d["dst"]): last_row_margin_mask(d["dst"]) for d in descs} if pad == 0 else None)


# ---------------------------------------------------------------------------------------------- 4
def keyable_source(w, sh, seed):
    """video noise with dark, colourless stretches (what black_key_feedback replaces) in pseudo-random padding"""
    fr = noise_frame(w, sh, seed)
    rng = np.random.RandomState(seed + 1)
    dark = rng.randint(0, 3, size=(sh, w // 2)) == 0
    fr.pix(0)[:, 0::2][dark] = rng.randint(10, 40, size=int(dark.sum()), dtype=np.uint8)
    fr.pix(0)[:, 1::2][dark] = rng.randint(10, 40, size=int(dark.sum()), dtype=np.uint8)
    for i in (1, 2):
        fr.pix(i)[dark] = rng.randint(120, 136, size=int(dark.sum()), dtype=np.uint8)
    return fr


def test_render_key_nocomp_and_positions():
    w, h = 96, 32
    sets = [L.make_params_tocomp(f) for f in (["-vhs"], ["-vhs", "-bkey-feedback", "3"], ["-bkey-feedback", "40"])]
    assert [s.black_key_level_feedback for s in sets] == [-1, 3, 40]
    src_flags = [0, _capi.F422_SRC420, _capi.F422_INTERLACED | _capi.F422_TFF, _capi.F422_SECOND,
                 _capi.F422_SRC420 | _capi.F422_INTERLACED | _capi.F422_SECOND, _capi.F422_INTERLACED]
    src_heights = [32, 48, 48, 50, 64, 40]
    explicit = {4: 1000, 7: 20, 11: 250000, 12: 0}        # (forwards, backwards, far, the very start)
    descs = []
    for k in range(18):
        fl = src_flags[k % 6] | (_capi.F422_NOCOMP if k % 3 == 1 else 0)
        descs.append(desc(k % 3 if k < 9 else (k // 3) % 3, fill_frame(w, h, 300 + k), (k & 1) ^ 1, k,
                          src=keyable_source(w, src_heights[k % 6], 400 + k), flt=fill_frame(w, h, 500 + k), flags=fl,
                          pos=explicit.get(k)))
    # the position does not move for a descriptor that does not composite
    p_of = lambda s: sets[s]
    for k in (1, 4, 10):
        assert descs[k]["flags"] & _capi.F422_NOCOMP
        assert oracle_run(p_of, [dict(descs[k], dst=descs[k]["dst"].copy(), flt=descs[k]["flt"].copy(), pos=77)], w, h, 0) == 77
    names = mixed_vs_oracle(sets, descs, w, h, start=123)
    assert names == NAMES_ALL          # (six fields of 16 rows per set: two workgroups each, so the halo kernel runs)
    # rows of a NOCOMP descriptor are the rendered (and keyed) rows: its set's noise has not touched them
    d = descs[1]
    ref = fill_frame(w, h, 301)
    L.tocomp_oracle_render_field(ref, keyable_source(w, src_heights[1], 401), 1, 0, 0, 0, d["field"])
    L.tocomp_oracle_black_key(ref, fill_frame(w, h, 501), d["field"], 3)
    assert np.array_equal(ref.buf, d["dst"].buf)
    # ... and the key did replace something in this content, and left the feedback of the set without it alone
    assert not np.array_equal(d["flt"].buf, fill_frame(w, h, 501).buf)
    assert np.array_equal(descs[0]["flt"].buf, fill_frame(w, h, 500).buf)


# ---------------------------------------------------------------------------------------------- 5
def forty_sets():
    sets = []
    for i in range(40):
        sets.append(L.make_params_tocomp(
            ["-vhs"], video_noise=(0 if i % 9 == 8 else 1 + 2 * i), video_chroma_noise=(0 if i % 7 == 6 else 3 + 37 * i),
            video_chroma_phase_noise=(i % 6) * 4, vhs_out_sharpen=0.25 + 0.125 * i, vhs_out_sharpen_chroma=0.1 * (i % 11),
            vhs_head_switching_phase=(0.1 + 0.0004 * i) if i % 2 else (0.97 + 0.0005 * i)))
    return sets


@pytest.mark.parametrize("own", [False, True], ids=["all_named", "half_on_the_ctx"])
def test_one_set_per_field(own):
    w, h = 96, 32
    sets = forty_sets()
    descs = [desc(-1 if own and k % 2 == 0 else k, noise_frame(w, h, 600 + k), (k & 1) ^ 1, k) for k in range(40)]
    names = mixed_vs_oracle(sets, descs, w, h, ctx_flags=["-vhs"], start=9)
    # (the twenty fields on the ctx's own parameters are one group of 320 rows: six workgroups, so the halo kernel runs)
    assert names == ["k_mixed_setup"] + (["k422_mixed_halo"] if own else []) + ["k422_mixed_process"]


# ---------------------------------------------------------------------------------------------- 6
def test_refusals_write_nothing_and_leave_the_position():
    torch = torch_mod()
    w, h = 64, 32
    lib = L.product()
    good = [L.make_params_tocomp(["-vhs"]), L.make_params_tocomp([])]
    ctx_params = L.make_params_tocomp(["-vhs", "-vhs-speed", "ep"])
    sim = ntscsim.FieldSimulator(params=ctx_params)
    sim.rng_pos = 4242

    padded = [noise_frame(w, h, 700 + k) for k in range(3)]
    tight = [noise_frame(w, h, 710 + k, 0) for k in range(2)]
    src = noise_frame(w, 24, 720)
    wide = noise_frame(2 * w + 8, h, 730)                 # two views of it that DO overlap: offset 8 pixels
    frames = padded + tight + [src, wide]
    dev = {}
    for fr in frames:
        whole = torch.from_numpy(fr.buf.copy()).cuda()
        dev[id(fr)] = (whole, [whole[fr.off[i]:fr.off[i] + fr.ls[i] * fr.h].view(fr.h, fr.ls[i]) for i in range(3)])

    def job(fr, field, fieldno=0, **kw):
        return dict({"dst": dev[id(fr)][1], "field": field, "fieldno": fieldno}, **kw)

    def call(set_of, jobs, sets=good, n_sets=None, width=w, height=h, n=None, edit=None):
        arr = sim.build_mixed_descs422(set_of, jobs)
        if edit:
            edit(arr)
        sarr = ntscsim.FieldSimulator.build_sets422(list(sets)) if sets is not None else None
        ns = (0 if sets is None else len(sets)) if n_sets is None else n_sets
        return lib.ntscsim_mixed_fields422_device(sim._h, sarr, ns, arr, len(arr) if n is None else n, width, height,
                                                  C.c_void_p(sim._torch_stream()))

    def bad_set(**kw):
        return L.make_params_tocomp(["-vhs"], **kw)

    def set_field(name, idx, v):
        def edit(arr):
            getattr(arr[0].d, name)[idx] = v
        return edit

    short = bad_set()
    short.struct_size -= 8
    ov_a = [p[:, 0:w] if i == 0 else p[:, 0:w // 2] for i, p in enumerate(dev[id(wide)][1])]
    ov_b = [p[:, 8:8 + w] if i == 0 else p[:, 4:4 + w // 2] for i, p in enumerate(dev[id(wide)][1])]
    two = [job(padded[0], 1), job(padded[1], 0, 1)]
    # (No case for "more than 2^30 rows": the limit cannot be reached through the ABI -- 65535 fields of at most 8192 rows
    #  stay below it, group padding included -- so tests/mixed_plan422_check.cpp holds the plan to it instead.)
    cases = [
        # --- what ntscsim_fields422_device refuses
        ("odd width", _capi.E_SIZE, lambda: call([0], [job(padded[0], 1)], width=w - 1)),
        ("width below 16", _capi.E_SIZE, lambda: call([0], [job(padded[0], 1)], width=14)),
        ("width above 16384", _capi.E_SIZE, lambda: call([0], [job(padded[0], 1)], width=16386)),
        ("height below 2", _capi.E_SIZE, lambda: call([0], [job(padded[0], 1)], height=1)),
        ("height above 16384", _capi.E_SIZE, lambda: call([0], [job(padded[0], 1)], height=16385)),
        ("field > 1", _capi.E_ARG, lambda: call([0, 1], [job(padded[0], 1), job(padded[1], 2)])),
        ("NULL plane", _capi.E_ARG, lambda: call([0], [job(padded[0], 1)], edit=set_field("dst_dev", 2, None))),
        ("short luma linesize", _capi.E_SIZE, lambda: call([0], [job(padded[0], 1)], edit=set_field("dst_linesize", 0, w - 1))),
        ("short chroma linesize", _capi.E_SIZE, lambda: call([1], [job(padded[0], 1)], edit=set_field("dst_linesize", 1, w // 2 - 1))),
        ("short source linesize", _capi.E_SIZE,
         lambda: call([0], [job(padded[0], 1, src=dev[id(src)][1], src_height=24)], edit=set_field("src_linesize", 0, w - 2))),
        ("NULL source plane", _capi.E_SIZE,
         lambda: call([0], [job(padded[0], 1, src=dev[id(src)][1], src_height=24)], edit=set_field("src_dev", 1, None))),
        ("short feedback linesize", _capi.E_SIZE,
         lambda: call([0], [job(padded[0], 1, flt=dev[id(padded[2])][1])], sets=[bad_set(black_key_level_feedback=3)],
                      edit=set_field("flt_linesize", 2, 3))),
        ("short src_height", _capi.E_SIZE, lambda: call([0], [job(padded[0], 1, src=dev[id(src)][1], src_height=1)])),
        ("short interlaced src_height", _capi.E_SIZE,
         lambda: call([0], [job(padded[0], 1, src=dev[id(src)][1], src_height=3, flags=_capi.F422_INTERLACED)])),
        ("n > 65535", _capi.E_SIZE, lambda: call([0] * 65536, [job(padded[0], 1)] * 65536)),
        ("n < 0", _capi.E_ARG, lambda: call([0], [job(padded[0], 1)], n=-1)),
        # --- the sets
        ("set below -1", _capi.E_ARG, lambda: call([0, -2], two)),
        ("set == n_sets", _capi.E_ARG, lambda: call([0, 2], two)),
        ("n_sets < 0", _capi.E_ARG, lambda: call([-1, -1], two, n_sets=-1)),
        ("NULL sets that should hold something", _capi.E_ARG, lambda: call([-1, 0], two, sets=None, n_sets=1)),
        ("wrong struct_size", _capi.E_ARG, lambda: call([0, 1], two, sets=[good[0], short])),
        ("a set the validator refuses", _capi.E_PARAM, lambda: call([1, 0], two, sets=[good[0], bad_set(video_noise=-1)])),
        ("a tape speed the validator refuses", _capi.E_PARAM, lambda: call([0, 1], two, sets=[good[0], bad_set(output_vhs_tape_speed=7)])),
        ("video_yc_recombine 65", _capi.E_PARAM, lambda: call([0, 1], two, sets=[good[0], bad_set(video_yc_recombine=65)])),
        ("video_yc_recombine -1", _capi.E_PARAM, lambda: call([0, 1], two, sets=[good[0], bad_set(video_yc_recombine=-1)])),
        # --- destinations, across the sets
        ("both fields of a tight-row frame, two sets", _capi.E_ARG, lambda: call([0, 1], [job(tight[0], 1), job(tight[0], 0, 1)])),
        ("both fields of a tight-row frame, set and ctx", _capi.E_ARG, lambda: call([-1, 1], [job(tight[1], 0), job(tight[1], 1, 1)])),
        ("the same frame and field twice, two sets", _capi.E_ARG,
         lambda: call([0, 1, 0], [job(padded[0], 1), job(padded[1], 1), job(padded[0], 1, 2)])),
        ("overlapping frames that are no side-by-side views", _capi.E_ARG,
         lambda: call([0, 1], [dict(dst=ov_a, field=1, fieldno=0), dict(dst=ov_b, field=0, fieldno=1)])),
    ]
    def untouched(what):
        """after a sync: every device buffer still holds its pristine host copy"""
        sim.sync()
        for k, fr in enumerate(frames):
            assert np.array_equal(dev[id(fr)][0].cpu().numpy(), fr.buf), "%s: wrote buffer %d" % (what, k)

    # after EACH refusal: the code, the position, and every buffer
    for what, want, fn in cases:
        rc = fn()
        assert rc == want, (what, rc)
        assert sim.rng_pos == 4242, what
        untouched(what)
    # n == 0 succeeds and does nothing
    assert call([], [], sets=good) == _capi.OK and sim.rng_pos == 4242
    untouched("n == 0")
    # a set nobody names is not looked at: this call is accepted (and does write its two fields)
    assert call([0, 0], two, sets=[good[0], bad_set(video_noise=-1)]) == _capi.OK
    sim.sync()
    assert sim.rng_pos == 4242 + calls422(good[0], w, h, 1) + calls422(good[0], w, h, 0)
    assert not np.array_equal(dev[id(padded[0])][0].cpu().numpy(), padded[0].buf)
    sim.close()
    # at the end, a valid call -- both fields of padded frames and side-by-side views, as the refused ones named them
    descs = [desc(0, padded[0], 1, 0), desc(1, padded[0], 0, 1), desc(1, padded[1], 1, 2), desc(-1, padded[2], 0, 3),
             desc(0, tight[0], 1, 4), desc(1, tight[1], 0, 5)]
    ctx = L.make_params_tocomp(["-vhs", "-vhs-speed", "ep"])
    c2 = Call(good, descs, w, h, ctx, 4242)
    sim = ntscsim.FieldSimulator(params=ctx)
    sim.rng_pos = 4242
    c2.enqueue(sim)
    pos = sim.rng_pos
    sim.sync()
    sim.close()
    assert pos == c2.end
    c2.check({id(fr): last_row_margin_mask(fr) for fr in tight})


# ---------------------------------------------------------------------------------------------- 7
def test_the_single_set_call_keeps_its_kernels_after_a_mixed_call():
    torch = torch_mod()
    w, h = 96, 32
    p = L.make_params_tocomp(["-vhs"])
    sim = ntscsim.FieldSimulator(params=p)
    o = L.TocompOracleStream(p, L.OOB_MEMORY)
    frame = noise_frame(w, h, 800)
    whole = torch.from_numpy(frame.buf.copy()).cuda()
    views = [whole[frame.off[i]:frame.off[i] + frame.ls[i] * h].view(h, frame.ls[i]) for i in range(3)]
    assert all(v.data_ptr() % 16 == 0 and v.stride(0) % 16 == 0 for v in views)          # aligned rows
    sim.fields422([{"dst": views, "field": 1, "fieldno": 0}], w, h)
    before = sim.last_kernels()
    o.process(frame, 1, 0)
    # a mixed call of other sets, -1 among them, in between
    sets = [L.make_params_tocomp(f) for f in ([], ["-vhs", "-vhs-speed", "lp", "-chroma-phase-noise", "7"])]
    descs = [desc(s, noise_frame(w, h, 810 + k), (k & 1) ^ 1, k) for k, s in enumerate([0, 1, -1, 1, 0])]
    call = Call(sets, descs, w, h, p, o.rng_pos)
    call.enqueue(sim)
    assert sim.last_kernels() == ["k_mixed_setup", "k422_mixed_process"]
    assert sim.rng_pos == call.end
    o = L.TocompOracleStream(p, L.OOB_MEMORY)
    o.skip(call.end)
    sim.fields422([{"dst": views, "field": 0, "fieldno": 1}], w, h)
    after = sim.last_kernels()
    o.process(frame, 0, 1)
    pos = sim.rng_pos
    sim.sync()
    got = whole.cpu().numpy()
    sim.close()
    assert after == before and any(k.startswith("k422_fused") for k in after), (before, after)
    assert pos == o.rng_pos
    assert np.array_equal(got, frame.buf)
    call.check()


# ---------------------------------------------------------------------------------------------- 8
def test_calls_in_flight_share_the_scratch():
    """two mixed calls of different layouts and sizes back to back on one ctx, nothing waited for in between: the second
    is laid out into the scratch the first still uses, behind it in stream order"""
    ctx = L.make_params_tocomp(["-vhs"])
    sets_a = [L.make_params_tocomp(f) for f in (["-vhs"], [], ["-vhs", "-vhs-speed", "ep"])]
    sets_b = [L.make_params_tocomp(f) for f in (["-vhs", "-vhs-svideo", "1"], ["-vhs"])]
    wa, ha, wb, hb = 96, 130, 64, 34
    descs_a = [desc([0, 1, 2, 0, 0, 2][k], noise_frame(wa, ha, 820 + k), (k & 1) ^ 1, k) for k in range(6)]
    descs_b = [desc([1, 0, 1, -1, 1][k], noise_frame(wb, hb, 840 + k), k & 1, 50 + k) for k in range(5)]
    a = Call(sets_a, descs_a, wa, ha, ctx, 3)
    b = Call(sets_b, descs_b, wb, hb, ctx, a.end)
    sim = ntscsim.FieldSimulator(params=ctx)
    sim.rng_pos = 3
    a.enqueue(sim)
    b.enqueue(sim)
    pos = sim.rng_pos
    sim.sync()
    sim.close()
    assert pos == b.end
    a.check()
    b.check()


# ---------------------------------------------------------------------------------------------- 9
def draw_layout(p):
    return (p.video_noise != 0, bool(p.vhs_head_switching and p.vhs_head_switching_phase_noise != 0),
            p.video_chroma_noise != 0, p.video_chroma_phase_noise != 0)


@pytest.mark.parametrize("first", ["bgra", "yuv422p"])
def test_the_table_cache_tells_the_two_tools_apart(first):
    """one ctx, the same W, H and draw layout through ntscsim_mixed_fields_device and ntscsim_mixed_fields422_device, in
    both orders: the jump tables differ (2 W against 2 (W/2) chroma draws per row), so each tool needs its own entry"""
    torch = torch_mod()
    w, h = 96, 32
    p_bgra = L.make_params(["-vhs"])
    p_422 = [L.make_params_tocomp(["-vhs"]), L.make_params_tocomp(["-vhs", "-vhs-svideo", "1"], vhs_out_sharpen=2.5)]
    assert draw_layout(p_bgra) == draw_layout(p_422[0]) == draw_layout(p_422[1]) == (True, True, True, True)
    assert p_bgra.video_chroma_phase_noise == p_422[0].video_chroma_phase_noise == p_422[1].video_chroma_phase_noise
    ctx = L.make_params_tocomp([])
    sim = ntscsim.FieldSimulator(params=ctx)
    # the BGRA call and its oracle
    srcs = [L.noise_frame(w, h, 0x345678 + j) for j in range(2)]
    exp = np.full((2, h, w, 4), 0x5A, np.uint8)
    src_t = torch.from_numpy(np.stack(srcs)).cuda()
    dst_t = torch.full((2, h, w, 4), 0x5A, dtype=torch.uint8, device="cuda")
    jobs = [(0, 0, 1, 0), (1, 1, 0, 1)]
    descs = [desc(k % 2, noise_frame(w, h, 860 + k), (k & 1) ^ 1, k) for k in range(4)]

    def run_bgra(start):
        o = L.OracleStream(p_bgra)
        o.skip(start)
        for (si, di, field, fieldno) in jobs:
            o.field(exp[di], srcs[si], field, fieldno)
        sim.rng_pos = start
        sim.mixed_fields([p_bgra], [0, 0], src_t, dst_t, jobs)
        assert sim.rng_pos == o.rng_pos
        return o.rng_pos

    def run_422(start):
        call = Call(p_422, descs, w, h, ctx, start)
        sim.rng_pos = start
        call.enqueue(sim)
        assert sim.rng_pos == call.end
        return call

    if first == "bgra":
        end = run_bgra(17)
        call = run_422(end)
    else:
        call = run_422(17)
        run_bgra(call.end)
    sim.sync()
    tables = sim.debug_mixed_tables()
    got = dst_t.cpu().numpy()
    sim.close()
    assert np.array_equal(got, exp)
    call.check()
    assert tables[0] == 2 and tables[1] == 1 and tables[2] == 0, tables


# ---------------------------------------------------------------------------------------------- 10
def test_profiling_covers_the_call():
    w, h = 96, 32
    ctx = L.make_params_tocomp([])
    sets = [L.make_params_tocomp(f) for f in (["-vhs"], [])]
    descs = [desc(k % 2, noise_frame(w, h, 880 + k), (k & 1) ^ 1, k) for k in range(4)]
    call = Call(sets, descs, w, h, ctx)
    sim = ntscsim.FieldSimulator(params=ctx)
    sim.set_profiling(True)
    call.enqueue(sim)
    sim.sync()
    t = sim.timings_ms()
    sim.close()
    assert t["calls"] == 1
    assert t["setup"] >= 0 and t["encode"] >= 0 and t["decode"] >= 0       # setup | (empty) | process
    assert t["total"] > 0 and t["total"] + 1e-3 >= t["setup"] + t["decode"]
    call.check()
