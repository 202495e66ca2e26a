"""The table of the YUV422P tool's role kernels (tests/_pipe422_forms.py) on the CPU: it names every role form the launcher can
note and nothing else, its widths stand on both sides of every loop condition of csrc/ntsc422_fused.hip (whose constants are
read out of that file here), and the oracle shows on every row what the row is for -- displaced rows of the claimed kind,
chroma rows lost and kept, nothing excluded from the comparison on padded rows, the rand() position.
"""
import os
import re

import numpy as np
import pytest

import _libs as L
import _pipe422_forms as T

CSRC = os.path.join(L.PKG, "csrc")
FUSED = open(os.path.join(CSRC, "ntsc422_fused.hip")).read()
LAUNCHER = open(os.path.join(CSRC, "ntscsim_hip.hip")).read()


# ------------------------------------------------------------------------------------------------ closure
def launcher_role_names():
    """the launcher's string literals that hold k422_pipe or k422_direct_pipe (its one error message about them is a sentence)"""
    lits = {s for s in T.string_literals(LAUNCHER) if "k422_pipe" in s or "k422_direct_pipe" in s}
    text = {s for s in lits if " " in s}
    assert text == {"k422_pipe: hand-off timed out in workgroup "}, text
    return sorted(lits - text)


def uncovered(rows):
    """role names of the launcher without a row, and role names of the rows the launcher does not hold"""
    have = {r.kernel for r in rows if r.kernel}
    names = launcher_role_names()
    return [n for n in names if n not in have], sorted(n for n in have if n not in names)


def test_every_role_name_of_the_launcher_has_a_row_and_every_row_a_name():
    names = launcher_role_names()
    assert names == sorted(T.ROLE_NAMES), names
    assert uncovered(T.ROWS) == ([], [])
    assert uncovered(T.SYNC) == ([], [])
    # the check bites: without the rows of one name that name is reported
    for n in T.ROLE_NAMES:
        assert uncovered([r for r in T.ROWS if r.kernel != n]) == ([n], []), n
    # every one-wave name of a fallback row is a literal of the launcher as well
    lits = set(T.string_literals(LAUNCHER))
    assert {r.fallback for r in T.ROWS if r.fallback} <= lits


def test_the_rows_name_what_the_launchers_rule_gives():
    """launch422()'s conditions restated over the parameters (T.launcher_name): the role form or the fallback of every row"""
    for r in T.ROWS:
        role, one = T.launcher_name(T.params(r), T.aligned(r.w, r.layout), r.n)
        assert role == r.kernel, (r.id, role, one)
        if r.fallback:
            assert one == r.fallback, (r.id, one)
    for s in T.SYNC:
        assert T.launcher_name(L.make_params_tocomp(s.flags), True, 1)[0] == s.kernel, s.id
    for form in T.ROLE_NAMES:
        assert T.launcher_name(L.make_params_tocomp(T.BASE[form]), True, T.MAX_FIELDS + 1) == (None, T.ONE_WAVE[form])
    fall = [r for r in T.ROWS if r.kernel is None]
    assert {r.layout for r in fall} >= {"odd", "odd-chroma", "padded"} and any(r.n == T.MAX_FIELDS + 1 for r in fall)


# ------------------------------------------------------------------------------------------------ the kernels' constants
def test_the_named_expressions_are_the_kernels_constants():
    """XR, the edge prologue's 8, HB, the steady loop's condition and sweep A's group loop as they stand in the source: a
    change there fails here until the table follows"""
    role = FUSED[FUSED.index("void k422_pipe("):FUSED.index("void k422_short(")]
    short_role = FUSED[FUSED.index("void k422_short_pipe("):]
    assert [int(x) for x in re.findall(r"constexpr int XR = (\d+);", role)] == [T.XR]
    assert set(re.findall(r"constexpr int HB = (\d+);", role + short_role)) == {str(T.HB)}
    # front and back: the same prologue, the same steady condition, the same trip
    pro = re.findall(r"for \(; i < (\d+) && i < NIT; i\+\+\) edge\(i\);", role)
    assert pro == [str(T.EDGE)] * 2, pro
    cond = re.findall(r"if \(i == (\d+) && i \+ (\d+) <= W2 - (\d+) - DD\)", role)
    assert cond == [(str(T.EDGE), str(T.STEP - 1), "2")] * 2, cond
    loop = re.findall(r"for \(; i \+ (\d+) <= W2 - (\d+) - DD; i \+= (\d+)\)", role)
    assert loop == [(str(T.STEP - 1), "2", str(T.STEP))] * 2, loop
    assert re.findall(r"NIT = W2 \+ DD \+ (\d+);", role) == ["2", "2"]
    assert "w - XR + 1 + DD" in role                                   # the ring's room: the back reads words i and i - DD
    # sweep A: groups of 32 chroma inputs, the guard-free form, the publish
    assert re.findall(r"for \(int g0 = 0; g0 < W2 \+ D; g0 \+= (\d+)\)", FUSED) == [str(T.GROUP)]
    assert re.findall(r"if \(FAST && g0 >= (\d+) && g0 \+ (\d+) <= W2\)", FUSED) == [(str(T.GROUP), str(T.GROUP))]
    assert "const int done = 2 * (g0 - D);" in role and "const int done = 2 * (g0 - 4);" in short_role
    assert re.findall(r"const int gidx = blockIdx\.x \* (\d+) \+ lane - 1;", role) == [str(T.WG_ROWS)]
    pipe = open(os.path.join(CSRC, "ntsc_pipe.hip")).read()
    assert re.findall(r"#define NTSC_PIPE_MAX_FIELDS (\d+)", pipe) == [str(T.MAX_FIELDS)]
    assert [T.steady_first(d) for d in (4, 5, 6)] == [34, 36, 38]
    assert [T.ring_last(d) for d in (4, 5, 6)] == [52, 50, 48]
    assert (T.groups_edge(1), T.groups_edge(2), T.groups_edge(1, True)) == (56, 120, 60)
    assert (T.fast_first(1), T.fast_first(2)) == (128, 192)


# ------------------------------------------------------------------------------------------------ coverage
def missing_conditions(rows, form):
    """the conditions of the issue's list that the widths of a form's rows (role form reached, padded rows) leave one-sided"""
    dd = T.DD[form]
    mine = [r for r in rows if r.kernel == form]
    ws = sorted({r.w for r in mine})
    ntsc = sorted({r.w for r in mine if "pal" not in r.flags})
    pal = sorted({r.w for r in mine if "pal" in r.flags})
    miss = []

    def both(what, pred, over):
        if {bool(pred(w)) for w in over} != {False, True}:
            miss.append(what)

    def edge(what, last, over):
        """the last width on one side and the first on the other"""
        if last not in over or last + 2 not in over:
            miss.append("%s %d|%d" % (what, last, last + 2))

    both("steady", lambda w: T.steady(w, dd), ws)
    edge("steady", T.steady_first(dd) - 2, ws)
    if not {T.HB, T.HB + 2} <= set(ws):
        miss.append("edge iterations only")
    above = [w for w in ws if T.steady(w, dd) and w < T.steady_first(dd) + 2 * T.STEP + 2]
    if {T.epilogue_class(w, dd) for w in above} != set(range(T.STEP)):
        miss.append("epilogue classes")
    both("ring", lambda w: T.ring_wraps(w, dd), ws)
    edge("ring", T.ring_last(dd), ws)
    for k in (1, 2):
        edge("groups", T.groups_edge(k), ntsc)
        if {T.a_groups(T.groups_edge(k)), T.a_groups(T.groups_edge(k) + 2)} != {k, k + 1}:
            miss.append("group count")
        for w in (T.fast_first(k) - 2, T.fast_first(k), T.fast_first(k) + 2):
            if w not in ntsc:
                miss.append("guard-free group %d" % w)
        if (T.a_fast_groups(T.fast_first(k) - 2), T.a_fast_groups(T.fast_first(k))) != (k - 1, k):
            miss.append("guard-free count")
    both("first publish", T.a_publishes_early, ntsc)
    if form not in (T.P_SPEC, T.P_DIRECT):                   # (sweep_a<false>: the forms that take PAL)
        edge("PAL groups", T.groups_edge(1, True), pal)
    if not {0, 2, T.HB - 2} <= {w % T.HB for w in ws}:
        miss.append("W mod 16")
    if not {0, 2, T.BURST - 2} <= {w % T.BURST for w in ws}:
        miss.append("W mod 64")
    if T.FULL not in ws:
        miss.append("full width")
    return miss


@pytest.mark.parametrize("form", T.ROLE_NAMES)
def test_widths_stand_on_both_sides_of_every_loop_condition(form):
    assert missing_conditions(T.ROWS, form) == []
    # the check bites: without a threshold width the condition is reported
    dd = T.DD[form]
    for w, what in ((T.steady_first(dd), "steady"), (T.steady_first(dd) - 2, "steady"), (T.ring_last(dd) + 2, "ring"),
                    (T.groups_edge(1), "groups"), (T.fast_first(1), "guard-free"), (T.FULL, "full width")):
        got = missing_conditions([r for r in T.ROWS if r.w != w], form)
        assert any(m.startswith(what) for m in got), (form, w, got)
    # ... and without the widths of one residue class that class
    for mod, what in ((T.HB, "W mod 16"), (T.BURST, "W mod 64")):
        for res in (0, 2, mod - 2):
            got = missing_conditions([r for r in T.ROWS if r.w % mod != res], form)
            assert what in got, (form, mod, res, got)
            if mod == T.HB:
                assert "W mod 64" in got                   # (a class mod 16 holds one mod 64)


# ------------------------------------------------------------------------------------------------ switch coverage
def permitted(form, tag):
    """launch422()'s rule on the switch sets a listed switch can be added to: does the form keep the launch?"""
    flags = dict((t, f) for t, f, _ in T.LISTED)[tag]
    for base in T.BASES[form]:
        p = L.make_params_tocomp(flags + base if tag == "pal" else base + flags)
        if T.launcher_name(p, True, 2)[0] == form:
            return True
    return False


def missing_switches(rows, form):
    """the listed switches a form's conditions allow that its rows do not hold at every width class"""
    pred = dict((t, f) for t, _, f in T.LISTED)
    mine = [(r, T.params(r)) for r in rows if r.kernel == form and r.layout == "padded" and not r.hs]
    miss = []
    for tag in T.ALL_LISTED:
        if not permitted(form, tag):
            continue
        have = {r.w for r, p in mine if pred[tag](p)}
        want = set(T.SWITCH_W) | (set(T.PAL_W) if tag == "pal" else set())
        if not want <= have:
            miss.append(tag)
    return miss


@pytest.mark.parametrize("form", T.ROLE_NAMES)
def test_every_form_holds_every_switch_its_conditions_allow(form):
    assert tuple(t for t in T.ALL_LISTED if permitted(form, t)) == T.PERMITS[form]
    assert missing_switches(T.ROWS, form) == []
    # the check bites: without the rows that hold a switch at one width class that switch is reported
    pred = dict((t, f) for t, _, f in T.LISTED)
    for tag in T.PERMITS[form]:
        for w in T.SWITCH_W:
            cut = [r for r in T.ROWS if not (r.kernel == form and r.w == w and pred[tag](T.params(r)))]
            assert len(cut) < len(T.ROWS) and tag in missing_switches(cut, form), (form, tag, w)


@pytest.mark.parametrize("form", T.ROLE_NAMES)
def test_rows_pack_into_the_workgroups_as_the_table_says(form):
    mine = [r for r in T.ROWS if r.kernel == form]
    lslot = lambda r: (r.h + 1) // 2
    total = lambda r: r.n * lslot(r)
    assert any(r.h == 2 for r in mine) and {9, 33} <= {r.h for r in mine}
    three = sorted((r.h, lslot(r), total(r)) for r in mine if r.n == 3 and r.w == T.ROWS_W)
    assert three == [(125, 63, 189), (126, 63, 189), (127, 64, 192)]          # R crosses 63 and 126: the halo lanes
    big = [r for r in mine if r.n == T.MAX_FIELDS]
    assert big and all((total(r) + T.WG_ROWS - 1) // T.WG_ROWS == 6 for r in big)
    assert any(r.share and r.source == "inplace" for r in mine) and any(r.share and r.source == "src" for r in mine)
    assert {r.layout for r in mine} == {"padded", "tight"} and all(r.w >= T.BURST and r.w % 16 == 0 for r in mine if r.layout == "tight")
    assert any(r.source == "src" for r in mine)
    over = [r for r in T.ROWS if r.fallback == T.ONE_WAVE[form] and r.n == T.MAX_FIELDS + 1]
    assert len(over) == 1
    hs = {(r.hs, r.w) for r in mine if r.hs and r.layout == "padded"}
    assert hs == {(k, w) for k in T.HS_KINDS for w in T.hs_widths(T.DD[form])}
    assert not T.steady(T.hs_widths(T.DD[form])[0], T.DD[form]) and T.steady(T.hs_widths(T.DD[form])[1], T.DD[form])


def test_sources_of_every_kind_are_in_the_table():
    assert {"src420", "src-il"} <= {r.source for r in T.ROWS}
    assert any(r.source == "src" and r.layout == "tight" for r in T.ROWS)


# ------------------------------------------------------------------------------------------------ the oracle on the rows
@pytest.mark.parametrize("row", T.ROWS, ids=lambda r: r.id)
def test_the_oracle_shows_what_the_row_is_for(row):
    c = T.case(row.id)
    p = T.params(row)
    # the rand() position is the sum of the product's closed form
    assert c.rng_pos == c.calls and c.rng_pos > 0, (c.rng_pos, c.calls)
    # what the comparison leaves out: nothing on padded rows; on tight rows at most the margin of one luma row and its two
    # chroma rows per frame
    out = int((~c.mask).sum())
    if row.layout == "tight":
        assert row.w >= T.BURST and 0 < out <= (24 + 14 + 14) * len(c.frames)
    else:
        assert out == 0
    # the launch touches the rows of its fields and nothing else: the other field's rows (unless both are in the launch),
    # padding and guards are as they were
    changed = c.init != c.exp
    assert changed.any()
    for j, f in enumerate(c.frames):
        e = T.frame_at(changed, j, row.w, row.h, row.layout)
        fields = {fld for (fi, _, fld, _, _) in c.jobs if fi == j}
        for i in range(3):
            width = row.w if i == 0 else row.w // 2
            assert not e.plane(i)[:, width:].any(), (j, i)
            for fld in {0, 1} - fields:
                assert not e.plane(i)[fld::2].any(), (j, i, fld)
        assert not e.buf[e.off[2] + e.ls[2] * row.h:].any(), j
    # head switching: displaced rows of the claimed kind beside undisplaced ones, in every field
    if row.hs:
        lim = row.w // 10
        for sh in c.shifts:
            moved = [s for s in sh if s]
            assert moved and sh.count(0) >= 2, (row.id, sh)
            if row.hs == "fwd":
                assert all(s > 0 for s in moved)
            elif row.hs == "back":
                assert all(-lim <= s < 0 for s in moved)
            else:
                assert min(moved) < -lim and all(s < 0 for s in moved)
                assert row.hs == "wide" or min(moved) == -lim - 1, sh
    else:
        assert not any(s for sh in c.shifts for s in sh), row.id
    # dropout: chroma rows lost and chroma rows kept
    if p.video_chroma_loss >= 1000:
        lost = kept = 0
        for (fi, _, fld, _, _) in c.jobs:
            e = T.frame_at(c.exp, fi, row.w, row.h, row.layout)
            for y in range(fld, row.h, 2):
                gone = (e.pix(1)[y] == 128).all() and (e.pix(2)[y] == 128).all()
                lost, kept = lost + gone, kept + (not gone)
        assert lost >= 1 and kept >= 1, (row.id, lost, kept)


def test_the_displacements_are_the_oracles():
    """T.hs_shifts() restates ffmpeg_to_composite.cpp:669-732 over the oracle's rand() stream.  Against the oracle itself:
    with the jitter of the switch off (no draws: both runs see the same stream) the rows that head switching changes are the
    rows the restatement displaces (a row's luma depends on no other row then), for every kind and width of the table's head-switch rows."""
    seen = set()
    for row in T.ROWS:
        if not row.hs or (row.hs, row.w) in seen or row.layout != "padded":
            continue
        seen.add((row.hs, row.w))
        # (the VCR's vertical chroma blend off: it carries a displaced row's chroma into the row below)
        quiet = row.flags + ["-vhs-head-switching-noise-level", "0", "-vhs-chroma-vblend", "0"]
        on = L.make_params_tocomp(quiet)
        off = L.make_params_tocomp(quiet + ["-vhs-head-switching", "0"])
        assert on.vhs_head_switching and not off.vhs_head_switching
        for field in (1, 0):
            buf = np.empty(T.frame_bytes(row.w, row.h, "padded"), np.uint8)
            a = T.frame_at(buf, 0, row.w, row.h, "padded")
            T.fill(buf, [a], 77 + row.w)
            b = a.copy()
            oa, ob = L.TocompOracleStream(on, L.OOB_MEMORY), L.TocompOracleStream(off, L.OOB_MEMORY)
            sh = T.hs_shifts(on, oa.g, row.w, row.h, field)
            oa.process(a, field, 0)
            ob.process(b, field, 0)
            assert oa.rng_pos == ob.rng_pos
            differ = [bool((a.pix(0)[y] != b.pix(0)[y]).any()) for y in range(field, row.h, 2)]
            assert differ == [s != 0 for s in sh], (row.id, field, sh, differ)
    assert len(seen) == len(T.HS_KINDS) * len({w for d in (4, 5, 6) for w in T.hs_widths(d)})
