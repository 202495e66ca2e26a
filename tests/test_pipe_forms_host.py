"""The table of the BGRA tool's role kernels in double (tests/_pipe_forms.py) on the CPU: it names every role form the launcher
can note and nothing else, its widths stand on both sides of every loop condition of csrc/ntsc_pipe.hip (whose constants are
read out of that file here), its packing rows pack as they claim, and the oracle shows on every row what the row is for --
the rand() position, untouched rows, displaced rows of the claimed class (from the oracle's own taps), chroma rows lost and
kept.  The launcher's rule, restated over ntscsim_params, names every row's kernel or fallback.
"""
import os
import re

import numpy as np
import pytest

import _libs as L
import _pipe_forms as T
import ntscsim

CSRC = os.path.join(L.PKG, "csrc")
PIPE = open(os.path.join(CSRC, "ntsc_pipe.hip")).read()
LAUNCHER = open(os.path.join(CSRC, "ntscsim_hip.hip")).read()


# ------------------------------------------------------------------------------------------------ closure
def launcher_role_names():
    """the launcher's string literals that begin with k_field_pipe and hold `double` (its error message about a hand-off that
    timed out begins alike and names no type)"""
    return sorted({s for s in T.string_literals(LAUNCHER) if s.startswith("k_field_pipe") and "double" in s})


def uncovered(rows):
    """role names of the launcher without a row, and role names of the rows the launcher does not hold"""
    have = {r.kernel for r in rows if r.kernel}
    names = launcher_role_names()
    return [n for n in names if n not in have], sorted(n for n in have if n not in names)


def test_every_role_name_of_the_launcher_has_a_row_and_every_row_a_name():
    names = launcher_role_names()
    assert names == sorted(T.ROLE_NAMES) and len(names) == 7, names
    assert uncovered(T.ROWS) == ([], [])
    assert uncovered(T.SYNC) == ([], [])
    # the check bites: without the rows of one name that name is reported
    for n in T.ROLE_NAMES:
        assert uncovered([r for r in T.ROWS if r.kernel != n]) == ([n], []), n
    # the float twins are literals of the launcher too (the GPU file asserts them by name)
    assert set(T.FLOAT_NAME.values()) <= set(T.string_literals(LAUNCHER))
    assert all((r.kernel is None) != (r.fallback is None) for r in T.ROWS)


# ------------------------------------------------------------------------------------------------ the kernels' constants
def test_the_named_expressions_are_the_kernels_constants():
    """RING, the field limit, the rows of a workgroup, the steady condition, the decoder's depth, the encoder's chunk end and
    its `more` as they stand in the source: a change there fails here until the table follows"""
    assert re.findall(r"constexpr int RING = (\d+);", PIPE) == [str(T.RING)]
    assert re.findall(r"#define NTSC_PIPE_MAX_FIELDS (\d+)", PIPE) == [str(T.MAX_FIELDS)]
    assert re.findall(r"const int gidx = blockIdx\.x \* (\d+) \+ R\.lane - 1;", PIPE) == [str(T.WG_ROWS)] * 2
    cond = re.findall(r"DEV bool has_steady\(int W, int d, int SKT\) \{ return SKT \+ (\d+) <= W - \(d > (\d+) \? d - (\d+) : 0\); \}", PIPE)
    assert cond == [(str(T.STEP), "7", "7")], cond
    assert re.findall(r"C\.SKT = \(sv \? (\d+) : (\d+)\) \+ C\.d;", PIPE) == [("8", "15")]
    assert "C.d = 0; C.SKT = 8;" in PIPE                                        # the TV front
    assert re.findall(r"const int t_end = W - \(C\.d > 7 \? C\.d - 7 : 0\);", PIPE) and "const int t_end = W - (d > 7 ? d - 7 : 0);" in PIPE
    assert len(re.findall(r"for \(; t \+ 4 <= t_end; t \+= 4\)", PIPE)) >= 4     # SEP (a macro), CHR, LUM, OUT
    assert re.findall(r"const int t_e = (\d+) \+ (\d+) \* \(\(W - (\d+)\) / (\d+)\);", PIPE) == [("4", "16", "4", "16")]
    assert (T.HEAD, T.CHUNK) == (4, 16)
    assert re.findall(r"const bool chunks = (\d+) \+ (\d+) <= W;", PIPE) == [("4", "16")]
    assert re.findall(r"const bool more = t \+ (\d+) <= W;", PIPE) == [str(2 * T.CHUNK)]
    assert "sbase = (sbase + 16) & 31;" in PIPE                                 # the rand() ring's halves
    assert "const int xb = xo & ~15;" in PIPE and "const int sub = (xo0 >> 2) & 3;" in PIPE
    assert "if (mn < -(W / 10)) return W;" in PIPE and "return (mx > 0 ? mx : 0) + 2;" in PIPE
    assert "if (!WR || !P.hs) return W / 10 + 2;" in PIPE
    assert re.findall(r"if \(W < (\d+) \|\| H < 2", LAUNCHER)[:1] == [str(T.MIN_W)]
    assert [T.steady_first(d, False) for d in (9, 12, 14)] == [30, 36, 40]
    assert [T.steady_first(d, True) for d in (9, 12, 14)] == [23, 29, 33]
    assert T.steady_first(0, False, True) == 12 < T.MIN_W
    for d, sv, tv in ((9, False, False), (14, True, False), (0, False, True)):
        s = T.steady_first(d, sv, tv)
        assert T.has_steady(s, d, sv, tv) and not T.has_steady(s - 1, d, sv, tv)
    assert [T.enc_chunks(w) for w in (19, 20, 35, 36, 51, 52, 67, 68)] == [0, 1, 1, 2, 2, 3, 3, 4]


# ------------------------------------------------------------------------------------------------ coverage
def width_rows(rows, f):
    return [r for r in rows if r.id.startswith(f.tag + "_w") and r.kernel == f.kernel and r.h == 10 and r.n == 2]


def missing_conditions(rows, f):
    """the conditions of the kernels' loops that the width rows of a family leave one-sided"""
    ws = sorted({r.w for r in width_rows(rows, f)})
    k = (f.d, f.sv, f.tv)
    s = T.steady_first(*k)
    miss = []

    def both(what, pred):
        if {bool(pred(w)) for w in ws} != {False, True}:
            miss.append(what)

    def edge(what, last):
        if last not in ws or last + 1 not in ws:
            miss.append("%s %d|%d" % (what, last, last + 1))

    if s > T.MIN_W:
        both("steady", lambda w: T.has_steady(w, *k))
        edge("steady", s - 1)
        if s - 2 not in ws:
            miss.append("steady %d" % (s - 2))
    elif not all(T.has_steady(w, *k) for w in ws) or T.MIN_W not in ws:
        miss.append("steady at the narrowest frame")
    above = [w for w in ws if T.has_steady(w, *k)]
    pairs = {(T.flush_class(w, *k), T.drain_class(w, *k)) for w in above}
    for fc in range(4):
        for dc in range(4):
            if (fc, dc) not in pairs:
                miss.append("flush %d drain %d" % (fc, dc))
    if {w & 1 for w in above} != {0, 1}:
        miss.append("parity of xe")
    if not {0, 1, 2} <= {min(T.trips(w, *k), 2) for w in ws} and s > T.MIN_W:
        miss.append("trips 0, 1, more")
    if not {False, True} == {4 * T.trips(w, *k) > T.RING for w in above}:
        miss.append("ring slots used once and again")
    edge("chunks", 19)
    edge("more", 35)
    edge("third chunk", 51)
    edge("fourth chunk", 67)
    both("more", T.enc_more)
    if not {0, 1, 2, 3} <= {min(T.enc_chunks(w), 3) for w in ws}:
        miss.append("chunk counts")
    for t in (0, 1, 15):
        if t not in {T.enc_tail(w) for w in ws}:
            miss.append("tail %d" % t)
    if T.FULL not in ws:
        miss.append("full width")
    # the list of widths itself: twenty consecutive widths from two below the threshold, the encoder's widths
    lo = T.first_width(f)
    miss.extend("width %d" % w for w in sorted(set(range(lo, lo + 20)) | set(T.ENC_W)) if w not in ws)
    return miss


@pytest.mark.parametrize("f", T.FAMILIES, ids=lambda f: f.tag)
def test_widths_stand_on_both_sides_of_every_loop_condition(f):
    assert missing_conditions(T.ROWS, f) == []
    ws = sorted({r.w for r in width_rows(T.ROWS, f)})
    lo = T.first_width(f)
    assert set(range(lo, lo + 20)) <= set(ws) and set(T.ENC_W) <= set(ws)
    # the check bites: without any one width of the table something is reported
    for w in ws:
        assert missing_conditions([r for r in T.ROWS if r.w != w], f), (f.tag, w)
    # ... without the widths on one side of a condition that condition, by name
    s = T.steady_first(f.d, f.sv, f.tv)
    for w, what in ((s - 1, "steady"), (s, "steady"), (19, "chunks"), (20, "chunks"), (35, "more"), (36, "more"), (52, "third chunk"),
                    (68, "fourth chunk"), (T.FULL, "full width")):
        if w >= T.MIN_W:
            got = missing_conditions([r for r in T.ROWS if r.w != w], f)
            assert any(m.startswith(what) for m in got), (f.tag, w, got)
    # ... and without the widths of one (flush, drain) class that class
    k = (f.d, f.sv, f.tv)
    for fc in range(4):
        for dc in range(4):
            cut = [r for r in T.ROWS if not (T.has_steady(r.w, *k) and (T.flush_class(r.w, *k), T.drain_class(r.w, *k)) == (fc, dc))]
            assert "flush %d drain %d" % (fc, dc) in missing_conditions(cut, f)


def test_the_families_cover_every_form_and_delay():
    fams = {(f.kernel, f.d) for f in T.FAMILIES}
    assert {(T.K_PLAIN, d) for d in (9, 12, 14)} | {(T.K_SV, d) for d in (9, 12, 14)} | {(T.K_WR, 9), (T.K_WR, 14)} <= fams
    assert {(T.K_XI, 9), (T.K_XI, 14), (T.K_CATV, 9), (T.K_CATV, 14), (T.K_TV, 0), (T.K_TVC, 0)} <= fams
    assert sum(f.kernel == T.K_XI for f in T.FAMILIES) == 3 and any(f.pal for f in T.FAMILIES if f.kernel == T.K_XI)
    for f in T.FAMILIES:
        p = L.make_params(T.fam_flags(f, 36))
        assert T.loop_consts(p) == (f.d, f.sv, f.tv), f.tag
        assert (p.tv_standard == 1) == f.pal
    # PAL's default switching point on the plain families: the wrap-around form without a displaced row
    assert {r.w for r in T.ROWS if r.id.startswith("wr_pal_sp_")} == {29, 30, 31, 100}
    assert {r.w for r in T.ROWS if r.id.startswith("wr_pal_ep_")} == {39, 40, 41, 100}


# ------------------------------------------------------------------------------------------------ switches
@pytest.mark.parametrize("tag", T.SWITCH_FAMILIES)
def test_every_form_holds_the_switches_its_condition_allows(tag):
    f = T.FAM[tag]
    mine = [(r, T.params(r)) for r in T.ROWS if r.id.startswith(tag + "_") and r.kernel]
    for sw, flags_of, pred in T.SWITCHES:
        if flags_of(f) is None:
            continue
        have = {r.w for r, p in mine if pred(p) and (sw == "pal" or r.kernel == f.kernel)}
        assert set(T.SWITCH_W) <= have, (tag, sw, have)
    s = T.steady_first(f.d, f.sv, f.tv)
    assert T.SWITCH_W[1] >= s and T.enc_chunks(T.SWITCH_W[2]) >= 3


def test_the_rows_that_must_fall_back_are_in_the_table():
    fall = [r for r in T.ROWS if r.kernel is None]
    P = {r.id: T.params(r) for r in fall}
    assert sum(r.n == T.MAX_FIELDS + 1 for r in fall) == len(T.PACK_FAMILIES)
    assert any(P[r.id].nocolor_subcarrier for r in fall)
    assert any(P[r.id].vhs_svideo_out and P[r.id].video_scanline_phase_shift == 90 for r in fall)
    assert any(P[r.id].composite_preemphasis and P[r.id].video_chroma_noise == 5 and not P[r.id].emulating_vhs for r in fall)
    assert any(P[r.id].video_noise == 0 and P[r.id].emulating_vhs for r in fall) and any(P[r.id].video_noise == 0 and not P[r.id].emulating_vhs for r in fall)
    assert any(not P[r.id].composite_out_chroma_lowpass_lite for r in fall) and any(not P[r.id].composite_out_chroma_lowpass for r in fall)
    assert any(P[r.id].ghost_taps for r in fall) and set(T.GHOST) <= {r.id for r in fall}
    assert set(T.DEBUG) <= {r.id for r in fall} and T.DEBUG and set(T.UNALIGNED) <= {r.id for r in fall} and T.UNALIGNED
    assert all(T.row_pixels(r) * 4 % 16 == (4 if r.id in T.UNALIGNED else 0) and T.row_pixels(r) > r.w for r in T.ROWS)


# ------------------------------------------------------------------------------------------------ packing
@pytest.mark.parametrize("tag", T.PACK_FAMILIES)
def test_rows_pack_into_the_workgroups_as_the_table_says(tag):
    f = T.FAM[tag]
    mine = [r for r in T.ROWS if r.id.startswith(tag + "_pack_") and r.kernel == f.kernel]
    assert {(r.w, r.h, r.n) for r in mine if r.h > 10} == {(w, h, n) for w in T.PACK_W for h in T.PACK_H for n in (1, 2, 3)}
    assert {T.lslot(h) for h in T.PACK_H} == {62, 63, 64, 65}
    straddle = midfield = blend_off = notok = 0
    for r in mine:
        for wg in range(T.workgroups(r.h, r.n)):
            ln = T.lanes(r.h, r.n, wg)
            straddle += len({f_ for (_, f_, _, _) in ln[1:]}) == 2
            midfield += ln[1][2] > 0
            blend_off += any(k < 2 and lane >= 2 for lane, (_, _, k, _) in enumerate(ln))
            notok += any(not ok for (_, _, _, ok) in ln[1:])
    assert straddle and midfield and blend_off and notok, (straddle, midfield, blend_off, notok)
    # odd heights: the last row of the slot is no row of the picture in the parity that starts at row 1
    for r in mine:
        if r.h & 1:
            assert any(f_ == 0 and k == T.lslot(r.h) - 1 and not ok
                       for wg in range(T.workgroups(r.h, r.n)) for (_, f_, k, ok) in T.lanes(r.h, r.n, wg)[1:])
    big = [r for r in mine if r.n == T.MAX_FIELDS]
    assert len(big) == 1 and T.workgroups(big[0].h, big[0].n) == 6
    over = [r for r in T.ROWS if r.id.startswith(tag + "_pack_") and r.n == T.MAX_FIELDS + 1]
    assert len(over) == 1 and over[0].kernel is None and over[0].fallback == T.ONE_LAUNCH[f.kernel]
    assert T.has_steady(36, f.d, f.sv, f.tv) and T.enc_chunks(100) == 6


# ------------------------------------------------------------------------------------------------ the oracle on the rows
def gray_rows(frame, field):
    """rows of a field whose pixels carry no chroma: B == G == R everywhere (a dropout zeroes I and Q of the whole row)"""
    px = frame[field::2].astype(np.int16)
    return [bool(((px[y, :, 0] == px[y, :, 1]) & (px[y, :, 1] == px[y, :, 2])).all()) for y in range(px.shape[0])]


@pytest.mark.parametrize("row", T.ROWS, ids=lambda r: r.id)
def test_the_oracle_shows_what_the_row_is_for(row):
    c = T.case(row.id)
    p = T.params(row)
    w, h = row.w, row.h
    # rand() is consumed, by the product's closed form
    calls = sum(ntscsim.calls_per_field(p, w, h, field) for (_, field, _) in c.jobs)
    assert c.rng_pos == calls, (c.rng_pos, calls)
    assert (calls > 0) == bool(p.video_noise or p.emulating_vhs), calls          # (the default preset's one draw is the luma noise)
    # a field's rows are written (alpha 0), the other field's rows, the padding and the guard frame are not
    for k, (_, field, _) in enumerate(c.jobs):
        assert (c.exp[k, 1 - field::2] == T.FILL).all() and (c.exp[k, :, w:] == T.FILL).all(), k
        assert not c.exp[k, field::2, :w, 3].any(), k
    assert (c.exp[row.n] == T.FILL).all()
    # head switching: the class the row claims, from the oracle's own taps
    flat = [s for sh in c.shifts for s in sh]
    lim = w // 10
    if row.hs is None:
        assert not any(flat), row.id
    elif row.hs == "none":
        assert not any(flat) and p.vhs_head_switching and not T.hs_small(p, w)
    elif row.hs == "small":
        assert all(any(sh) for sh in c.shifts) and all(abs(s) <= lim for s in flat) and T.hs_small(p, w), c.shifts
    elif row.hs == "fwd":
        assert all(max(sh) > lim and min(sh) == 0 for sh in c.shifts) and not T.hs_small(p, w), c.shifts
    else:
        assert all(min(sh) < -lim and max(sh) == 0 for sh in c.shifts) and not T.hs_small(p, w), c.shifts
    if row.hs:
        assert all(sh.count(0) >= 2 for sh in c.shifts)                     # displaced rows beside undisplaced ones
        branches = T.wg_branches(row, c.shifts)
        want = {"none": ["none"], "small": None, "fwd": ["fwd"], "wide": ["wide"], "last": ["none", "wide"]}[row.hs]
        assert want is None or branches == want * (1 if row.hs == "last" else len(branches)), branches
    # dropout: chroma rows lost and chroma rows kept
    if p.video_chroma_loss >= 1000:
        g = [x for k, (_, field, _) in enumerate(c.jobs) for x in gray_rows(c.exp[k, :, :w], field)]
        assert any(g) and not all(g), (row.id, g)
    # the composite tap holds a plane for every row of every field
    assert [t.shape for t in c.comp] == [(L.field_rows(h, field), w) for (_, field, _) in c.jobs]


def test_every_outcome_of_wg_reach_is_taken_on_every_form_with_wrap_around_loads():
    for kernel in T.WR_CAPABLE:
        seen, last = set(), 0
        for r in T.ROWS:
            if r.kernel == kernel and r.hs:
                b = T.wg_branches(r, T.case(r.id).shifts)
                seen.update(b)
                last += r.hs == "last" and b == ["none", "wide"] and T.workgroups(r.h, r.n) == 2
        assert seen == {"none", "fwd", "wide"} and last >= 2, (kernel, seen, last)
    # the forms without wrap-around loads keep displacements within W/10, in either direction
    for kernel in (T.K_PLAIN, T.K_TV, T.K_TVC):
        sh = [s for r in T.ROWS if r.kernel == kernel and r.hs == "small" for f in T.case(r.id).shifts for s in f]
        assert sh and (kernel == T.K_TVC or (min(sh) < 0 < max(sh))), (kernel, sh)


def test_the_displacements_read_off_the_taps_are_the_switches():
    """T.displacements() against the switch that made them: the first displaced row moves by the hx T.hs_flags() asked for
    (the jitter is below half a sample at these widths), the rows below by 7/8 of the row above, truncated"""
    for r in T.ROWS:
        if r.hs in ("fwd", "wide", "last") and r.w <= 100 and "_hs_" in r.id:
            tw = r.w + r.w // 10
            hx = r.w // 10 + max(2, r.w // 8) if r.hs == "fwd" else -(r.w // 10 + max(3, r.w // 5))
            for sh in T.case(r.id).shifts:
                moved = sh[next(i for i, s in enumerate(sh) if s):]
                want, s = [], hx
                while len(want) < len(moved):
                    want.append(s)
                    s = int(s * 7 / 8)
                assert moved == want and abs(hx) < tw // 2, (r.id, sh)


# ------------------------------------------------------------------------------------------------ the launcher's rule
def test_the_rows_name_what_the_launchers_rule_gives():
    """launch_records()'s conditions restated over the parameters (T.launcher_name): the role form or the fallback of every row"""
    for r in T.ROWS:
        role, one = T.launcher_name(T.params(r), r.w, r.n, aligned=r.id not in T.UNALIGNED, debug=T.DEBUG.get(r.id, 0),
                                    ghost=len(T.GHOST.get(r.id, ())))
        assert role == r.kernel, (r.id, role, one)
        if r.fallback:
            assert one == r.fallback, (r.id, one)
        # without the latency form, and in a launch of 65 fields, no row takes a role kernel
        assert T.launcher_name(T.params(r), r.w, r.n, latency=False)[0] is None
        assert T.launcher_name(T.params(r), r.w, T.MAX_FIELDS + 1)[0] is None
    for s in T.SYNC:
        assert T.launcher_name(L.make_params(s.flags), s.w, 1)[0] == s.kernel, s.id
    assert {s.kernel for s in T.SYNC} == set(T.ROLE_NAMES) and all(sum(s.kernel == k for s in T.SYNC) == 3 for k in T.ROLE_NAMES)
    for k in T.ROLE_NAMES:
        mine = sorted((s.w, s.h) for s in T.SYNC if s.kernel == k)
        p = L.make_params(next(s.flags for s in T.SYNC if s.kernel == k))
        first = T.steady_first(*T.loop_consts(p))
        assert mine[2] == (T.FULL, 486) and mine[0][0] == max(T.MIN_W, first - 1) and mine[1][0] == max(T.MIN_W + 1, first), (k, mine)
