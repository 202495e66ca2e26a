"""The table of the YUV422P tool's sweep kernels (tests/_sweep422_forms.py) on the CPU: it names every form launch422() can
note beside the role and the streamed kernels and nothing else, the restated launcher rule predicts every row's name, its
widths stand on both sides of every loop condition of csrc/ntsc422_kernels.hip and csrc/ntsc422_fused.hip (whose constants
are read out of those files here) per form, chroma delay and alignment combination, every listed switch is on every form
whose rule allows it, and the oracle shows on every row what the row is for -- the rand() position, the other field's rows
untouched, displaced rows of the claimed kind, chroma rows lost and kept, and how little the comparison leaves out.
"""
import os
import re

import numpy as np
import pytest

import _libs as L
import _pipe422_forms as T
import _sweep422_forms as S

CSRC = os.path.join(L.PKG, "csrc")
KERNELS = open(os.path.join(CSRC, "ntsc422_kernels.hip")).read()
FUSED = open(os.path.join(CSRC, "ntsc422_fused.hip")).read()
LAUNCHER = open(os.path.join(CSRC, "ntscsim_hip.hip")).read()
LAUNCH422 = LAUNCHER[LAUNCHER.index("static int launch422("):LAUNCHER.index('extern "C" int ntscsim_fields422_device(')]


@pytest.fixture(scope="module")
def facts():
    """per row: (parameters, (luma aligned, chroma aligned), delay class) -- computed once"""
    out = {}
    for r in S.ROWS:
        p = S.params(r)
        out[r.id] = (p, S.alignment(r.w, r.h, r.layout), S.delay_key(p))
    return out


# ------------------------------------------------------------------------------------------------ closure
def closure_names():
    """launch422()'s string literals that are neither role names (tests/_pipe422_forms.py's) nor streamed names"""
    lits = {s for s in T.string_literals(LAUNCH422) if s.startswith("k422_")}
    assert set(S.STREAMED) <= lits and {s for s in lits if "pipe" in s} == set(T.ROLE_NAMES)
    return sorted(s for s in lits if "pipe" not in s and s not in S.STREAMED)


def names_of(rows):
    have = {r.kernel for r in rows}
    if any(r.source in ("src", "src420", "src-il") for r in rows):
        have.add("k422_render")
    if any(r.source == "bkey" for r in rows):
        have.add("k422_bkey")
    return have


def uncovered(rows):
    have, names = names_of(rows), closure_names()
    return [n for n in names if n not in have], sorted(n for n in have if n not in names)


def test_every_name_of_the_launcher_has_rows_and_every_row_a_name():
    assert closure_names() == sorted(S.FORMS + ("k422_render", "k422_bkey"))
    assert uncovered(S.ROWS) == ([], [])
    assert not {r.kernel for r in S.ROWS} & set(S.STREAMED) and not any("pipe" in r.kernel for r in S.ROWS)
    # the check bites: without the rows of one name that name is reported
    for n in S.FORMS:
        assert uncovered([r for r in S.ROWS if r.kernel != n]) == ([n], []), n
    assert uncovered([r for r in S.ROWS if r.source == "inplace"]) == (["k422_bkey", "k422_render"], [])
    assert S.MIXED_NAME in T.string_literals(LAUNCHER)


def test_the_rows_name_what_the_launchers_rule_gives(facts):
    """launch422()'s conditions restated over the parameters, the two alignments and the debug bits (S.launcher_rule): the
    name of every row, of its companion launch, and of every reach on every layout the table says it holds on"""
    for r in S.ROWS:
        p, (ay, ac), _ = facts[r.id]
        assert S.launcher_rule(p, ay, ac, r.bits) == r.kernel, r.id
        other = S.launcher_rule(p, ay, ac, S.companion_bits(r))
        assert other in S.STREAMED + S.FORMS and (other != r.kernel or r.kernel == S.PROC), (r.id, other)
        assert r.bits == S.REACH[r.reach].bits and r.kernel == S.REACH[r.reach].form
    combos = {"padded": (True, True), "odd": (False, False), "odd-chroma": (True, False), "odd-luma": (False, True)}
    for reach in S.REACHES:
        p = L.make_params_tocomp(reach.flags)
        for lay, (ay, ac) in combos.items():
            name = S.launcher_rule(p, ay, ac, reach.bits)
            assert (name == reach.form) == (lay in reach.layouts), (reach.tag, lay, name)
        if not reach.bits:
            assert reach.layouts in (S.ANY, S.UNALIGNED)
    # which forms the dispatcher reaches on its own, and which only the debug bits reach
    own = {(r.kernel, facts[r.id][1]) for r in S.ROWS if r.bits == 0}
    assert {k for k, _ in own} == {S.PROC, S.F4, S.DIRECT}
    assert (S.F4, (True, True)) not in own and {a for k, a in own if k == S.F4} == {(False, False), (True, False), (False, True)}
    assert {a for k, a in own if k == S.DIRECT} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {r.bits for r in S.ROWS if r.kernel == S.S4} == {4}
    assert {r.bits for r in S.ROWS if r.kernel == S.F4} == {0, 2, 4} and {r.bits for r in S.ROWS if r.kernel == S.DIRECT} == {0, 2}


# ------------------------------------------------------------------------------------------------ the kernels' constants
def test_the_named_expressions_are_the_kernels_constants():
    """the conditions as they stand in the two sources: a change there fails here until the table follows"""
    body = KERNELS[KERNELS.index("DEV void process422_body("):]
    assert re.findall(r"constexpr int BK = (\d+);", KERNELS) == [str(S.BK)]
    assert re.findall(r"for \(; x0 \+ (\d+) <= W; x0 \+= (\d+)\)", body) == [("16", "16"), ("64", "64"), ("16", "16")]
    assert re.findall(r"for \(; c0 \+ (\d+) <= W2; c0 \+= (\d+)\)", body) == [("8", "8"), ("32", "32"), ("8", "8")]
    assert (S.VEC_Y, S.VEC_C, S.BURST_Y, S.BURST_C) == (16, 8, 64, 32)
    assert body.count("if (P.src_al16)") == 2 and body.count("if (P.dst_al16)") == 2          # in-copy and out-copy, each on its own
    assert re.findall(r"const int gidx = \(int\)blk \* (\d+) \+ lane - 1;", body) == [str(S.WG_ROWS)]
    assert set(re.findall(r"const int gidx = blockIdx\.x \* (\d+) \+ lane - 1;", FUSED)) == {str(S.WG_ROWS)}
    # the gathers: tw and the steps
    assert "const int tw = W + W / 10;" in body and "for (int x0 = 0; x0 < W; x0 += BK)" in body
    four = FUSED[FUSED.index("void k422_fused("):FUSED.index("void k422_pipe(")]
    short = FUSED[FUSED.index("void k422_short("):FUSED.index("void k422_short_pipe(")]
    for text in (four, short):
        assert "const int tw = W + W / 10;" in text and "for (int x0 = 0; x0 < W; x0 += HB)" in text
        assert re.findall(r"constexpr int HB = (\d+);", text) == [str(S.HB)]
    # the low-passes' delays (Packer422::finish(W2 - delay)), the VCR's chroma delay and its raw taps
    assert "const uint32_t mask = (1u << (8 * (n & 3))) - 1u;" in KERNELS
    assert KERNELS.count("out.finish(W2 > delay ? W2 - delay : 0);") == 2
    assert body.count("chroma_lp_full422(R.U, W2, P.a_in_i, a_hp_i, 2);") == 2
    assert body.count("P.ntsc ? a_hp_q : a_hp_i, P.ntsc ? 4 : 2);") == 2 and body.count("chroma_lp_plain422(R.U, W2, P.a_tv, 1);") == 1
    assert S.LP_DELAYS == (1, 2, 4)
    speeds = re.findall(r"D\.cdelay = (\d+);", LAUNCHER[LAUNCHER.index("D.cdelay = 4;"):][:400])
    assert [int(x) for x in speeds] == [S.DELAYS["sp"], S.DELAYS["lp"], S.DELAYS["ep"]]
    for text in (body, FUSED[FUSED.index("DEV void sweep_b2("):FUSED.index("struct StreamB")]):
        assert "const int rawU = d == 4 ? wu[2] : (d == 5 ? wu[1] : wu[0]);" in text
        assert "int u = xo < W2 - d ? fU : rawU, v = xo < W2 - d ? fV : rawV;" in text
        assert "SWEEP_BEGIN(R.U, W2 + d)" in text
        assert "if (blend && k >= 1) {" in text and "u = ((k >= 2 ? upU : 128) + u + 1) >> 1;" in text and "__shfl_up(u, 1)" in text
    # the fused file's readers and sweep A
    assert "constexpr int B = 4 * NWB;" in FUSED and S.SB == 4 * 4
    assert FUSED.count("sweep_blocks<4>(R.Y, W + 2,") == 1
    assert "if (al16 && x0 + 16 <= n) {" in FUSED and "if (al8 && x0 + 8 <= n) {" in FUSED
    assert re.findall(r"for \(int g0 = 0; g0 < W2 \+ D; g0 \+= (\d+)\)", FUSED) == [str(S.GROUP)] and S.GROUP == T.GROUP
    assert "constexpr int D = NTSC ? 4 : 2, DU = 2, DV = NTSC ? 4 : 2;" in FUSED
    assert "typedef FrameSinkT<RowWriter<4>, RowWriter<2>> FrameSink;" in FUSED
    assert re.findall(r"if \(W < (\d+) \|\| \(W & 1\)", LAUNCHER[LAUNCHER.index("static int prepare422("):][:3000])[:1] == [str(S.MIN_W)]
    variant = open(os.path.join(os.path.dirname(__file__), "test_variant422.py")).read()
    assert re.findall(r"MARGIN_Y, MARGIN_C = (\d+), (\d+)", variant) == [(str(S.MARGIN_Y), str(S.MARGIN_C))]
    # what the widths are for
    assert [S.raw_window(S.MIN_W, d) for d in (4, 5, 6)] == [4, 3, 2]
    assert (S.groups_edge(1), S.groups_edge(2), S.groups_edge(1, True), S.groups_edge(2, True)) == (56, 120, 60, 124)
    assert {w % 64 for w in S.EVEN} == set(range(0, 64, 2)) and {w // 2 % 32 for w in S.EVEN} == set(range(32))
    assert {S.bursts(w) for w in S.EVEN} == {0, 1, 2} and {S.a_groups(w) for w in S.EVEN} == {1, 2, 3}
    assert [w // 10 for w in S.GATHER_W] == [1, 1, 2, 3, 4]


# ------------------------------------------------------------------------------------------------ coverage of the conditions
COMBOS = [(True, True), (False, False), (True, False), (False, True)]
# (form, delay class) and the alignment combinations its rule allows
WANT = [(S.PROC, k, c) for k in ("sp", "lp", "ep", "pal") for c in COMBOS] + \
       [(S.F4, k, c) for k in ("sp", "lp", "ep", "pal") for c in COMBOS] + [(S.S4, "sp", (True, True))] + \
       [(S.DIRECT, k, c) for k in ("novcr", "pal") for c in COMBOS]


def missing_conditions(rows, facts, form, key, combo):
    """the conditions of the table that the widths of a form's rows leave one-sided, for one delay class on one combination of
    luma and chroma alignment (rows of three fields in one workgroup: the families "w" and "edge")"""
    ws = sorted({r.w for r in rows if r.kernel == form and r.fam in ("w", "edge") and facts[r.id][1] == combo and facts[r.id][2] == key})
    miss = []
    if not ws:
        return ["no rows"]
    w2 = [w // 2 for w in ws]
    d = S.DELAYS.get(key)

    def classes(what, got, want):
        if not set(want) <= set(got):
            miss.append(what)

    def edge(what, last):
        if last not in ws or last + 2 not in ws:
            miss.append("%s %d|%d" % (what, last, last + 2))

    # (the input low-pass and the full output one, delays 2 and 4, are on in these rows; the lite one's delay 1 has a test below)
    for n, what in ((0, "finish(W2)"),) + tuple((k, "finish(W2 - %d)" % k) for k in S.LP_DELAYS[1:]):
        classes(what, {S.finish_class(v - n) for v in w2}, range(4))
    classes("finish(W)", {S.finish_class(w) for w in ws}, (0, 2))
    classes("ragged block of W2", {S.ragged(v) for v in w2}, range(S.BK))
    classes("ragged block of W", {S.ragged(w) for w in ws}, range(0, S.BK, 2))
    if d:
        classes("ragged block of W2 + d", {S.ragged(v + d) for v in w2}, range(S.BK))
        if min(S.raw_window(w, d) for w in ws) != S.raw_window(S.MIN_W, d):
            miss.append("smallest window")
    if S.MIN_W not in ws:
        miss.append("smallest width")
    classes("vector tail", {S.vec_tail(w) for w in ws}, (False, True))
    classes("byte block", {S.byte_block(w) for w in ws}, (False, True))
    classes("bursts", {S.bursts(w) for w in ws}, (0, 1, 2))
    for k in (1, 2):
        edge("bursts", k * S.BURST_Y - 2)
    classes("pieces", {S.pieces(w) for w in ws}, range(4))
    classes("ragged block of W + 2", {S.blocks_ragged(w) for w in ws}, (False, True))
    if form != S.PROC:
        pal = key == "pal"
        classes("groups", {S.a_groups(w, pal) for w in ws}, (1, 2, 3))
        for k in (1, 2):
            edge("groups", S.groups_edge(k, pal))
    if S.FULL not in ws:
        miss.append("full width")
    return miss


@pytest.mark.parametrize("form,key,combo", WANT, ids=lambda v: str(v).replace(" ", ""))
def test_widths_stand_on_both_sides_of_every_condition(facts, form, key, combo):
    assert missing_conditions(S.ROWS, facts, form, key, combo) == []
    # the check bites: without a threshold width, or the widths of a residue class, the condition is reported
    pal = key == "pal"
    cuts = [(lambda w: w == S.MIN_W, "smallest width"), (lambda w: w == S.BURST_Y, "bursts"), (lambda w: w == 2 * S.BURST_Y - 2, "bursts"),
            (lambda w: w % S.VEC_Y == 0, "vector tail"), (lambda w: w // 2 % 4 == 3, "finish(W2)"), (lambda w: w // 2 % 8 == 5, "ragged block of W2"),
            (lambda w: w % 64 // 16 == 3, "pieces"), (lambda w: w % 16 == 14, "ragged block of W + 2"), (lambda w: w == S.FULL, "full width")]
    if form != S.PROC:
        cuts += [(lambda w: w == S.groups_edge(1, pal), "groups"), (lambda w: w == S.groups_edge(2, pal) + 2, "groups")]
    for cut, what in cuts:
        got = missing_conditions([r for r in S.ROWS if not cut(r.w)], facts, form, key, combo)
        assert any(m.startswith(what) for m in got), (what, got)
    # ... and without a family of rows -- the reach that carries this class on this alignment -- everything is
    mine = {r.reach for r in S.ROWS if r.kernel == form and r.fam in ("w", "edge") and facts[r.id][1] == combo and facts[r.id][2] == key}
    assert missing_conditions([r for r in S.ROWS if r.reach not in mine], facts, form, key, combo) == ["no rows"]


def test_the_sweep_holds_every_even_width_per_form_and_delay(facts):
    want = set(S.EVEN + S.BIG)
    assert S.BIG == (190, 192, 194, 254, 256, 258, 718, 720, 722) and S.EVEN[0] == 16 and S.EVEN[-1] == 146 and len(S.EVEN) == 66
    for form, key in sorted({(f, k) for f, k, _ in WANT}):
        for al in ((True, True), (False, False)):
            if form == S.S4 and not al[0]:
                continue
            have = {r.w for r in S.ROWS if r.fam == "w" and r.kernel == form and facts[r.id][2] == key and facts[r.id][1] == al}
            assert have == want, (form, key, al, sorted(want - have))
    # small rows: H = 5 and H = 6, each field parity owns the last row once; three fields
    small = [r for r in S.ROWS if r.fam in ("w", "edge")]
    assert {r.h for r in small} == {5, 6} and {r.n for r in small} == {3}
    for form in S.FORMS:
        for lay in ("padded", "tight"):
            assert {r.h for r in small if r.kernel == form and r.layout == lay} == {5, 6}, (form, lay)
    # every reach of the table stands at the conditions' widths: on aligned rows where it holds there, on unaligned rows
    # where it holds on those alone -- and every reach of the twelve sweeps on both
    for reach in S.REACHES:
        for al in ((True, True), (False, False)):
            lay = "padded" if al[0] else "odd"
            if lay in reach.layouts and (al[0] or reach.form == S.PROC or "padded" not in reach.layouts):
                have = {r.w for r in small if r.reach == reach.tag and facts[r.id][1] == al}
                assert set(S.edge_widths()) <= have, (reach.tag, al)


def lite_widths(rows, facts, form, al):
    return {r.w for r in rows if r.kernel == form and r.fam == "edge" and facts[r.id][1] == al and T._out_lp(facts[r.id][0]) == 1}


@pytest.mark.parametrize("form", [S.PROC, S.F4, S.DIRECT])
def test_the_lite_low_pass_stands_at_the_conditions_widths(facts, form):
    """chroma_lp_plain422 (delay 1) runs for no switch set's default: its finish(W2 - 1) and FrameSink's mode 1 have rows of
    their own, on aligned and on unaligned rows, with and without the VCR where the form has both"""
    for al in ((True, True), (False, False)):
        ws = lite_widths(S.ROWS, facts, form, al)
        assert set(S.edge_widths()) <= ws, (form, al)
        assert {S.finish_class(w // 2 - S.LP_DELAYS[0]) for w in ws} == set(range(4))
    if form == S.PROC:
        lite = [r for r in S.ROWS if r.kernel == form and r.fam == "edge" and T._out_lp(facts[r.id][0]) == 1]
        assert {bool(facts[r.id][0].emulating_vhs) for r in lite} == {False, True}
    # the check bites: without the reaches that carry it nothing is left
    assert not lite_widths([r for r in S.ROWS if "lite" not in r.reach], facts, form, (True, True))
    # the preset instantiation cannot take it (its identity: the full output low-pass)
    assert not any(T._out_lp(facts[r.id][0]) != 2 for r in S.ROWS if r.kernel == S.S4)


# ------------------------------------------------------------------------------------------------ switch coverage
def permitted(reach, tag):
    """launch422()'s rule on a listed switch added to a reach's switch set: does the form keep the launch?"""
    p = L.make_params_tocomp(S.listed_flags(reach, tag))
    return S.launcher_rule(p, True, True, S.REACH[reach].bits) == S.REACH[reach].form


def missing_switches(rows, facts, form):
    """the listed switches a form's rule allows that its rows do not hold at every width class"""
    pred = dict((t, f) for t, _, f in S.LISTED)
    mine = [r for r in rows if r.kernel == form and r.layout == "padded" and not r.hs and r.fam.startswith("sw")]
    miss = []
    for tag in S.ALL_LISTED:
        if not any(permitted(t, tag) for t in S.SWITCH_REACH if S.REACH[t].form == form):
            continue
        have = {r.w for r in mine if pred[tag](facts[r.id][0])}
        if not set(S.SWITCH_W) <= have:
            miss.append(tag)
    return miss


@pytest.mark.parametrize("form", S.FORMS)
def test_every_form_holds_every_switch_its_rule_allows(facts, form):
    for t in S.SWITCH_REACH:
        assert tuple(x for x in S.ALL_LISTED if permitted(t, x)) == S.PERMITS[t], t
    assert {S.REACH[t].form for t in S.SWITCH_REACH} == set(S.FORMS)
    assert missing_switches(S.ROWS, facts, form) == []
    assert S.SWITCH_W[0] < 32 <= S.SWITCH_W[1] <= 146 and S.SWITCH_W[2] == S.FULL
    # the check bites: without the rows that hold a switch at one width class that switch is reported
    pred = dict((t, f) for t, _, f in S.LISTED)
    for tag in S.ALL_LISTED:
        if not any(permitted(t, tag) for t in S.SWITCH_REACH if S.REACH[t].form == form):
            continue
        for w in S.SWITCH_W:
            cut = [r for r in S.ROWS if not (r.kernel == form and r.w == w and r.fam.startswith("sw") and pred[tag](facts[r.id][0]))]
            assert len(cut) < len(S.ROWS) and tag in missing_switches(cut, facts, form), (form, tag, w)
    # the switches of the list that are no single predicate: the three output low-passes, the noises singly, both amplitudes,
    # the three phases with odd offsets, both pre-emphasis presets
    assert {"full", "lite", "nolp", "noblend", "drop", "amp30", "amp1", "catv", "catv3", "p0", "p90", "p270", "n0", "cn0", "pn0"} <= set(S.ALL_LISTED)


@pytest.mark.parametrize("form", S.FORMS)
def test_rows_pack_into_the_workgroups_as_the_table_says(form):
    mine = [r for r in S.ROWS if r.kernel == form]
    lslot = lambda r: (r.h + 1) // 2
    packs = {(lslot(r), r.n) for r in mine if r.fam == "rows" and not r.share}
    assert packs == {(ls, n) for ls in (62, 63, 64, 65) for n in (1, 2, 3)}
    # fields start on every lane class of the 63-row workgroups: the first row of field 1 and 2 is lane 1 + Lslot * k mod 63
    starts = {(k * ls) % S.WG_ROWS for ls, n in packs for k in range(n)}
    assert {0, 1, 2, 4, 61, 62} <= starts
    assert any(r.share and r.layout == "padded" and r.h >= 126 for r in mine) and any(r.share and r.h == 6 for r in mine)
    assert any(r.fam == "full" and r.h == 127 and r.n == 3 for r in mine)
    assert {r.source for r in mine} == {"inplace", "src", "src420", "src-il", "bkey"}
    assert sum(r.source == "bkey" for r in mine) == 1
    # head switching: every kind at every class of the gather, on the step of 8 and on the step of 16
    hs = {(r.hs, r.w) for r in mine if r.hs}
    assert hs == {(k, w) for k in S.HS_KINDS for w in S.HS_W}
    assert set(S.GATHER_W) <= set(S.HS_W) and S.FULL in S.HS_W
    assert len({S.gather_class(w) for w in S.HS_W}) == len(S.HS_W)


def test_what_may_be_excluded(facts):
    """Nothing on layouts with luma linesize >= W + 2; on tight rows the right margin of each frame's last row -- and every
    (form, width, switch family) with a tight row has a row on a layout that excludes nothing"""
    for r in S.ROWS:
        assert (T.linesizes(r.w, r.layout)[0] >= r.w + 2) == (r.layout != "tight")
    full = {(r.kernel, r.w, r.fam, tuple(r.flags)) for r in S.ROWS if r.layout != "tight"}
    tight = [r for r in S.ROWS if r.layout == "tight"]
    assert tight and {r.kernel for r in tight} == set(S.FORMS)
    for r in tight:
        assert any((r.kernel, r.w, fam, tuple(r.flags)) in full for fam in ("w", "edge")), r.id
    for m in S.MIXED:
        assert m.layout != "tight" or any(o.layout == "padded" and o.w == m.w for o in S.MIXED)


# ------------------------------------------------------------------------------------------------ the oracle on the rows
def check_row(row):
    c = S.case(row.id)
    p = S.params(row)
    # the rand() position is the sum of the product's closed form
    assert c.rng_pos == c.calls and c.rng_pos > 0, (c.rng_pos, c.calls)
    # what the comparison leaves out
    out = int((~c.mask).sum())
    if row.layout == "tight":
        assert 0 < out <= (S.MARGIN_Y + 2 * S.MARGIN_C) * len(c.frames)
    else:
        assert out == 0
    # the launch touches the rows of its fields and nothing else
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
        assert not e.buf[e.off[0] + e.ls[0] * row.h:e.off[1]].any() and not e.buf[e.off[2] + e.ls[2] * row.h:].any(), j
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
    # the black key: pixels replaced from the filter frame, the filter frame written
    if row.source == "bkey":
        assert (c.fltinit != c.fltexp).any()


@pytest.mark.parametrize("group", list(S.GROUPS), ids=str)
def test_the_oracle_shows_what_the_rows_are_for(group):
    rows = S.GROUPS[group]
    assert 0 < len(rows) <= S.GROUP_ROWS and len({(r.reach, r.bits) for r in rows}) == 1
    sets = [tuple(r.flags) for r in rows]                 # the rows of one switch set follow each other: one context each
    assert len({s for s in sets}) == 1 + sum(a != b for a, b in zip(sets, sets[1:]))
    for row in rows:
        check_row(row)


def test_every_row_is_in_one_group():
    ids = [r.id for rows in S.GROUPS.values() for r in rows]
    assert sorted(ids) == sorted(r.id for r in S.ROWS)


@pytest.mark.parametrize("m", S.MIXED, ids=lambda m: m.id)
def test_the_oracle_on_the_mixed_rows(m):
    c = S.mixed_case(m.id)
    assert len(c.sets) == 10 and all(c.set_of.count(s) == 2 for s in range(10))
    assert all(a != b for a, b in zip(c.set_of, c.set_of[1:]))
    for s in range(10):
        assert {fld for (i, _, fld, _, _), t in zip(c.jobs, c.set_of) if t == s} == {0, 1}, s     # one field of each parity
    keys = [S.delay_key(p) for p in c.sets]
    assert {"sp", "lp", "ep", "pal", "novcr"} <= set(keys) and sum(bool(p.vhs_svideo_out) for p in c.sets) == 1
    assert sum(p.video_yc_recombine == 1 for p in c.sets) == 1 and sum(bool(p.nocolor_subcarrier) for p in c.sets) == 1
    assert sum(bool(p.nocolor_subcarrier_after_yc_sep) for p in c.sets) == 1 and sum(not p.composite_in_chroma_lowpass for p in c.sets) == 1
    changed = c.init != c.exp
    for j, (i, _, fld, _, _) in enumerate(c.jobs):
        e = T.frame_at(changed, i, m.w, m.h, m.layout)
        assert e.plane(0)[fld::2].any() and not any(e.plane(k)[fld ^ 1::2].any() for k in range(3)), j
    out = int((~c.mask).sum())
    assert (0 < out <= (S.MARGIN_Y + 2 * S.MARGIN_C) * len(c.frames)) if m.layout == "tight" else out == 0
    # a group's rows: two fields; the field edge and the group's end lie inside workgroups of 63 rows
    lslot = (m.h + 1) // 2
    assert lslot % S.WG_ROWS and (2 * lslot) % S.WG_ROWS
    assert c.rng_pos > 0


def test_the_mixed_rows_are_the_issues():
    assert S.MIXED_W == tuple(range(16, 48, 2)) + (64, 66, 720)
    assert {m.layout for m in S.MIXED} == {"padded", "tight", "odd"} and len(S.MIXED) == 3 * len(S.MIXED_W)
    assert any(2 * ((m.h + 1) // 2) > S.WG_ROWS for m in S.MIXED)            # a group of two workgroups: k422_mixed_halo


def test_the_displacements_are_the_oracles():
    """T.hs_shifts() against the oracle itself at the widths of this table's head-switch rows (as the sibling's test)"""
    seen = set()
    for row in S.ROWS:
        if not row.hs or (row.hs, row.w) in seen or row.layout != "padded" or S.REACH[row.reach].form == S.DIRECT:
            continue
        seen.add((row.hs, row.w))
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
    assert len(seen) == len(S.HS_KINDS) * len(S.HS_W)
