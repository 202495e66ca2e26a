"""The table of FAST32 kernel forms (tests/_fast32_forms.py) on the CPU: the reference side of every row of
tests/test_fast32_forms_gpu.py exists and behaves, and the table names every `float` form the launcher can pick.

Per row the fast32 flavour of the mode model consumes exactly the oracle's draws, leaves the other field's rows and alpha
alone and stays within 1 LSB of the oracle (float filter states in place of double ones move a unit of the 256-scaled
signal here and there, never a whole output step more) -- tests/test_modes_oracle.py does this for every third small case
of tests/cases.py.  The closure test reads csrc/ntscsim_hip.hip: a float form added later without a row fails here.
"""
import ast
import os
import re

import numpy as np
import pytest

import _fast32_forms as F
import _libs as L
import _modes as M

CSRC = os.path.join(L.PKG, "csrc")


@pytest.mark.parametrize("row", F.ROWS + F.ROLES + F.NO_ROLE, ids=lambda r: r.id)
def test_fast32_model_draws_like_the_oracle_on_every_row(row):
    role = isinstance(row, F.Role)
    p = F.params(row.flags, () if role else row.ghost)
    w, h = row.w, row.h
    srcs = M.sources("mixed" if role else row.kind, w, h)
    il, tff = (0, 0) if role else (row.il, row.tff)
    o, m = L.OracleStream(p), M.ModelStream(p, "fast32")
    lo, hi = 255, 0
    for si, field, fieldno in M.jobs(4 if role else row.n, len(srcs)):
        a = np.zeros((h, w, 4), np.uint8)
        b = np.full((h, w, 4), 0x5A, np.uint8)
        o.field(a, srcs[si], field, fieldno, il, tff)
        m.field(b, srcs[si], field, fieldno, il, tff)
        assert m.rng_pos == o.rng_pos, (row.id, fieldno)
        assert (b[1 - field::2] == 0x5A).all() and not b[field::2, :, 3].any(), (row.id, fieldno)
        assert np.abs(a[field::2].astype(np.int16) - b[field::2].astype(np.int16)).max() <= 1, (row.id, fieldno)
        lo, hi = min(lo, int(b[field::2, :, :3].min())), max(hi, int(b[field::2, :, :3].max()))
    if not role and row.kind == "saturating":
        assert (lo, hi) == (0, 255), (row.id, lo, hi)           # both output clamps are hit


def test_every_family_has_a_saturating_and_a_decaying_row():
    fam = {}
    for r in F.ROWS:
        fam.setdefault((tuple(r.names), r.mode), set()).add(r.kind)
    short = {k: v for k, v in fam.items() if not {"saturating", "decay"} <= v}
    # the rows taken over from tests/cases.py keep that file's inputs; a chain that only they reach is listed here
    assert sorted(short) == sorted([
        ((F.ENC_PRE, F.G_TV), F.HT), ((F.ENC_G, F.DEC_TV), F.HT), ((F.ENC_G, F.G_TV), F.HT), ((F.ENC, F.G_TV), F.HT),
        ((F.ENC, F.G_VHS), F.HT), ((F.ENC_G, F.G_VHS), F.HT), ((F.ENC, F.GHOST, F.DEC_TV), F.HT),
        ((F.ENC, F.GHOST, F.DEC_TV), F.NOFOLD), ((F.GH2, F.DEC_TV), F.HT), ((F.GH4, F.DEC_VHS), F.HT)]), short


def test_decay_rows_are_what_the_table_says():
    w, h = 720, 16
    fr = M.decay(w, h)
    e = w // 8
    plain = [y for y in range(h) if y % 3 and y % 5]
    assert plain and (fr[plain, :e, 0] == 255).all() and (fr[plain, :e, 2] == 24).all() and not fr[plain, :e, 1].any()
    assert (fr[plain, w - e:, 1] == 255).all() and not fr[plain, e:w - e].any()
    assert (fr[0::5, :, :3] == 255).all() and not fr[3::15].any() and not fr[..., 3].any()
    assert w - 2 * e >= 500                                     # hundreds of black samples between the colours


def test_where_the_composite_tap_sits():
    """The composite_y tap against the plane the product exposes (the encoder's): the tap is taken in FRONT of the ghosting
    extension -- with taps set it is the tap of the same switches without them, while the frames differ -- and BEHIND
    composite pre-emphasis (it changes when only the pre-emphasis gain does).  So k_ghost rows and pre-emphasis rows
    compare the plane, rows with the ghosting folded into the encoder (which stores the ghosted plane) do not."""
    w, h = 68, 10
    src = L.noise_frame(w, h, 5)

    def run(p):
        d = np.zeros((h, w, 4), np.uint8)
        return M.ModelStream(p, "fast32").field(d, src, 1, 0, taps=["composite_y"])["composite_y"], d

    t0, d0 = run(F.params(F.VHS))
    t1, d1 = run(F.params(F.VHS, F.GHOST_FUSED[1]))
    assert np.array_equal(t0, t1) and not np.array_equal(d0, d1)
    p = F.params(["-comp-catv"])
    q = F.params(["-comp-catv"])
    q.composite_preemphasis = p.composite_preemphasis / 2
    assert not np.array_equal(run(p)[0], run(q)[0])
    for r in F.ROWS:
        assert r.plane == (not any(n.startswith("k_encode_fast_gh") for n in r.names)), r.id


def test_ghost_tap_lists_are_the_parity_tests():
    tree = ast.parse(open(os.path.join(L.ROOT, "tests", "test_gpu_parity.py")).read())
    val = [n.value for n in tree.body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "_GHOST_FUSED"]
    assert len(val) == 1 and ast.literal_eval(val[0]) == F.GHOST_FUSED


def test_float_mode_row_count_is_the_dispatchers_rule():
    """the rows NTSCSIM_MODE_FLOAT runs on its own kernels: the two presets' families and nothing else"""
    take = [r.id for r in F.ROWS if F.float_forms_take(r, F.params(r.flags, r.ghost))]
    assert len(take) == F.N_FLOAT_ROWS, take
    assert all(i.startswith(("def_", "sp_", "lp_", "ep_", "own_vhs_lp_only", "own_interlaced_")) for i in take), take


def test_the_table_holds_the_families_and_cases_it_is_for():
    ids = {(tuple(r.flags), r.mode): r for r in F.ROWS}
    for name in ("noise0", "chroma_noise_only", "phase_noise20", "nocolor", "nocolor_vhs", "amp30", "amp1", "no_outlp",
                 "no_inlp", "vhs_lp_only", "hs_nonoise", "interlaced_tff", "interlaced_bff"):
        g, o = F.BY_ID["gen_" + name], F.BY_ID["own_" + name]
        assert g.mode == F.GEN and g.names[0] == F.ENC_G and g.names[1] in (F.G_TV, F.G_VHS) and o.mode == F.HT
    assert (F.BY_ID["gen_interlaced_tff"].il, F.BY_ID["gen_interlaced_tff"].tff) == (1, 1)
    assert (F.BY_ID["gen_interlaced_bff"].il, F.BY_ID["gen_interlaced_bff"].tff) == (1, 0)
    assert (tuple(F.PAL), F.HT) in ids and ids[(tuple(F.PAL), F.HT)].names[1] == F.DEC_WR
    for fam in ("def", "sp", "lp", "ep", "xi_p90", "fo_sp", "bk_vhs_catv", "bk_tv_catv", "sv_sp", "two_sp", "gh2_sp", "gh4_def",
                "tpl_sp", "tpl_def", "tpl_sv", "gen_sp", "gen_def", "gen_sv"):
        for w in F.WIDTHS:
            assert "%s_%dx10" % (fam, w) in F.BY_ID
        assert fam + "_100x35" in F.BY_ID


# ------------------------------------------------------------------------------------------------ closure
def _launcher():
    return open(os.path.join(CSRC, "ntscsim_hip.hip")).read()


def _macro_names(text):
    """the float names launch_records() assembles from macro arguments, from the macro invocations themselves"""
    fl = dict((k, int(v)) for k, v in re.findall(r"\b(F_[A-Z]+)\s*=\s*(\d+)u", open(os.path.join(CSRC, "ntsc_kernels.hip")).read()))
    assert set(fl) >= {"F_GENERIC", "F_CNOISE", "F_PNOISE", "F_LNOISE"}

    def f(expr):
        expr = re.sub(r"F_[A-Z]+", lambda m_: str(fl[m_.group(0)]), expr).replace("u", "")
        assert re.fullmatch(r"[0-9|() ]+", expr), expr
        return eval(expr)

    # the pieces the names are assembled around
    for piece in ('"k_encode<"', '"k_decode<" #VHS "," #CO ","', '"k_decode_fast<" #VHS "," #RT ">"', '"k_decode_fast_bk<" #VHS "," #RT ">"',
                  '"k_decode_fast<true," #RT ",true>"', '"k_encode_fast_gh<"', '"u," #RT ">"'):
        assert piece in text, piece
    out = set()
    for fe in re.findall(r"NTSC_LAUNCH_ENCODE\((F_\w+), float\)", text):
        out.add("k_encode<%du,float>" % f(fe))
    # (NTSC_LAUNCH_DECODE picks RT from the mode: every invocation has a float twin)
    for vhs, co, fe in re.findall(r"NTSC_LAUNCH_DECODE\((true|false), (true|false), (.+?)\);", text):
        out.add("k_decode<%s,%s,%du,float>" % (vhs, co, f(fe)))
    for vhs in re.findall(r"NTSC_LAUNCH_FAST\((true|false), float\)", text):
        out.add("k_decode_fast<%s,float>" % vhs)
    for vhs in re.findall(r"NTSC_LAUNCH_FAST_BK\((true|false), float\)", text):
        out.add("k_decode_fast_bk<%s,float>" % vhs)
    if re.search(r"NTSC_LAUNCH_FAST_WR\(float\)", text):
        out.add("k_decode_fast<true,float,true>")
    for gt in re.findall(r"NTSC_LAUNCH_GH\(float, (\d+)\)", text):
        out.add("k_encode_fast_gh<float,%s>" % gt)
    return out


def test_the_table_names_every_float_form_of_the_launcher():
    text = _launcher()
    names = F.all_names()
    # every string literal that names a kernel and contains `float`
    lits = set(re.findall(r'"(k_[A-Za-z0-9_]+<[^"]*float[^"]*)"', text))
    assert len(lits) >= 15, lits
    assert not lits - names, sorted(lits - names)
    # the names assembled from macro arguments: the table's explicit list is the launcher's, and every one has a row
    assert _macro_names(text) == set(F.MACRO_NAMES), sorted(_macro_names(text) ^ set(F.MACRO_NAMES))
    assert not set(F.MACRO_NAMES) - names
    # nothing in the table that the launcher cannot name
    assert {n for n in names if "float" in n} == lits | set(F.MACRO_NAMES)
    assert set(F.ROLE_NAMES) == {n for n in lits if n.startswith("k_field_pipe")}
    assert {r.name for r in F.ROLES} == set(F.ROLE_NAMES)
    # every other kernel name a note_kernel() call can record is either a double twin or has no RT at all
    for n in set(re.findall(r'"(k_[A-Za-z0-9_]+(?:<[^"]*>)?)"', text)) - lits:
        assert "float" not in n
