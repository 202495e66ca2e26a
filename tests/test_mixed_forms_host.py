"""Which kernel form a group of an ntscsim_mixed_fields_device call takes under ntscsim_set_mixed_forms(NTSCSIM_MIXED_TUNED)
(csrc/mixed_forms.hpp: the rule and the block tables per form) has no HIP in it, so it is checked on the host:

  * tests/mixed_forms_check.cpp, a stand-alone program with its own main, is compiled with plain g++, and again with the
    address and undefined-behaviour sanitizers, and both are run as the programs they are;
  * ntscsim_debug_mixed_form_of reaches the rule as the library applies it (the set's switches read off ntscsim_params, the
    head-switch range, the plane of the WHOLE call), without a device: every row of tests/cases.py, and 720 x 486 with the
    call's field count on both sides of each threshold of ntscsim_debug_fast_plane_ok."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import pytest

import _libs as L
import cases
import ntscsim
from ntscsim import _capi

_FLAGS = {
    "plain": ["-O1"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}

# csrc/mixed_forms.hpp
ENC_GENERIC, ENC_FAST, ENC_FAST_PRE = 0, 1, 2
DEC_GEN_TV, DEC_GEN_VCR, DEC_GEN_SV, DEC_TV, DEC_VHS, DEC_VHS_WR, DEC_SV, DEC_BK_TV, DEC_BK_VHS = range(9)


@pytest.mark.parametrize("build", sorted(_FLAGS))
def test_form_tables_and_the_rule(tmp_path, build):
    """120 pseudo-random plans with random form assignments (every group's blocks exactly once, in its form's table, in
    order; sizes add up), the rule over all combinations of its facts against a second statement of it, and every
    precondition flipped on its own from six sets that take a hand-tuned form."""
    assert shutil.which("g++") is not None, "g++ is needed to build tests/mixed_forms_check.cpp"
    here = os.path.dirname(os.path.abspath(__file__))
    exe = tmp_path / ("mixed_forms_check_" + build)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + _FLAGS[build] +
                          ["-I", os.path.join(L.PKG, "csrc"), os.path.join(here, "mixed_forms_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    m = re.search(r"mixed_forms: (\d+) checks, (\d+) bad", r.stdout)
    assert r.returncode == 0 and m and int(m.group(1)) > 100000 and int(m.group(2)) == 0, r.stdout[-4000:]


def form_of(p, w, h, n_total, aligned=1, mode=_capi.MODE_EXACT):
    e, d = C.c_int(-1), C.c_int(-1)
    rc = ntscsim.lib().ntscsim_debug_mixed_form_of(C.byref(p), w, h, n_total, aligned, mode, C.byref(e), C.byref(d))
    assert rc == _capi.OK, rc
    return e.value, d.value


def head_switch_small(p, w):
    """every head-switch displacement of the set within w / 10 samples (ffmpeg_ntsc.cpp:1647-1684: the switching point
    in samples of the 1.1 w wide line, with the phase noise at both of its ends)"""
    if not p.vhs_head_switching:
        return True
    tw = w + w // 10
    t = tw * (262.5 if p.tv_standard == 0 else 312.5)
    pn = abs(p.vhs_head_switching_phase_noise)
    lo, hi = p.vhs_head_switching_phase - pn, p.vhs_head_switching_phase + pn
    if lo < 0 or math.trunc(lo) != math.trunc(hi):
        return False
    plo, phi = int((lo - math.trunc(lo)) * t), int((hi - math.trunc(hi)) * t)
    if plo // tw != phi // tw:
        return False
    a, b = plo % tw, phi % tw
    if (a >= tw // 2) != (b >= tw // 2):
        return False
    a, b = (a - tw if a >= tw // 2 else a), (b - tw if b >= tw // 2 else b)
    return max(abs(a), abs(b)) <= tw - w


def expected_forms(p, w, aligned=True):
    """The rule of the issue, from the public parameter struct, for a call whose plane is small: the form the single-set
    launcher documents for the set (README / DESIGN 3: which presets the hand-tuned kernels cover)."""
    vhs, sv = bool(p.emulating_vhs), bool(p.vhs_svideo_out)
    gen = DEC_GEN_TV if not vhs else (DEC_GEN_SV if sv else DEC_GEN_VCR)
    even = p.video_scanline_phase_shift in (0, 180) and p.video_scanline_phase_shift_offset % 2 == 0
    if not aligned or not even or p.subcarrier_amplitude != 50:
        return ENC_GENERIC, gen
    pre = p.composite_preemphasis != 0 and p.composite_preemphasis_cut > 0
    enc = ENC_GENERIC
    if p.composite_in_chroma_lowpass and p.video_noise != 0:
        enc = ENC_FAST_PRE if pre else ENC_FAST
    dec = gen
    back = p.subcarrier_amplitude_back
    lite = p.composite_out_chroma_lowpass and p.composite_out_chroma_lowpass_lite
    cn, pn = p.video_chroma_noise != 0, p.video_chroma_phase_noise != 0
    small = head_switch_small(p, w)
    if not p.nocolor_subcarrier and lite and (back == 50 or back >= 2):
        if vhs and cn and pn:
            if sv:
                dec = DEC_SV if back == 50 else gen
            else:
                dec = (DEC_VHS if small else DEC_VHS_WR) if back == 50 else DEC_BK_VHS
        elif not vhs and not cn and not pn and small:
            dec = DEC_TV if back == 50 else DEC_BK_TV
    return enc, dec


@pytest.mark.parametrize("case", cases.CASES, ids=[c[0] for c in cases.CASES])
def test_every_row_of_the_case_table(case):
    p = L.make_params(case[1])
    for mode in (_capi.MODE_EXACT, _capi.MODE_FAST32, _capi.MODE_FLOAT):
        assert form_of(p, 96, 32, 46, 1, mode) == expected_forms(p, 96)
    # a call with an unaligned row somewhere: generic forms of the set's class
    assert form_of(p, 96, 32, 46, 0) == expected_forms(p, 96, aligned=False)
    assert form_of(p, 96, 32, 46, 0)[0] == ENC_GENERIC and form_of(p, 96, 32, 46, 0)[1] < 3


def test_rows_the_issue_names():
    """a handful spelled out, so that the table above cannot agree with the rule by sharing a mistake"""
    want = {
        "default": (ENC_FAST, DEC_TV), "vhs": (ENC_FAST, DEC_VHS), "vhs_ep": (ENC_FAST, DEC_VHS),
        "vhs_svideo": (ENC_FAST, DEC_SV), "vhs_pal": (ENC_FAST, DEC_VHS_WR), "vhs_noblend": (ENC_FAST, DEC_VHS),
        # (a switching point moved into the frame displaces rows by more than a tenth of the width: the wrap-around form)
        "hs_neg": (ENC_FAST, DEC_VHS_WR), "hs_pos": (ENC_FAST, DEC_VHS_WR), "hs_nonoise": (ENC_FAST, DEC_VHS_WR),
        "catv4_vhs": (ENC_FAST_PRE, DEC_BK_VHS),
        "phase90": (ENC_GENERIC, DEC_GEN_VCR), "phase270": (ENC_GENERIC, DEC_GEN_VCR), "phase0": (ENC_GENERIC, DEC_GEN_TV),
        "vhs_full_outlp": (ENC_FAST, DEC_GEN_VCR), "no_outlp": (ENC_FAST, DEC_GEN_TV), "no_inlp": (ENC_GENERIC, DEC_TV),
        "nocolor_vhs": (ENC_FAST, DEC_GEN_VCR), "nocolor": (ENC_FAST, DEC_GEN_TV), "amp30": (ENC_GENERIC, DEC_GEN_VCR),
        "noise0": (ENC_GENERIC, DEC_TV), "chroma_noise_only": (ENC_GENERIC, DEC_GEN_TV), "phase_noise20": (ENC_FAST, DEC_GEN_TV),
    }
    flags = {c[0]: c[1] for c in cases.CASES}
    got = {n: form_of(L.make_params(flags[n]), 96, 32 if n != "vhs_pal" else 36, 46) for n in want}
    assert got == want


def test_refusals_of_the_hook():
    lib = ntscsim.lib()
    p = L.make_params(["-vhs"])
    e, d = C.c_int(), C.c_int()
    ok = (C.byref(p), 96, 32, 4, 1, 0, C.byref(e), C.byref(d))
    assert lib.ntscsim_debug_mixed_form_of(*ok) == _capi.OK
    for i, v in ((0, None), (1, 8), (2, 1), (3, 0), (5, 3), (5, -1), (6, None), (7, None)):
        a = list(ok)
        a[i] = v
        assert lib.ntscsim_debug_mixed_form_of(*a) == _capi.E_ARG, (i, v)
    ghost = L.make_params(["-vhs"], ghost_taps=1)
    ghost.ghost_delay[0], ghost.ghost_gain[0] = 8, 64
    assert lib.ntscsim_debug_mixed_form_of(C.byref(ghost), *ok[1:]) == _capi.E_PARAM
    assert lib.ntscsim_debug_mixed_form_of(C.byref(L.make_params([], video_noise=-1)), *ok[1:]) == _capi.E_PARAM


def last_ok(w, h, hs_mode):
    """the largest field count ntscsim_debug_fast_plane_ok admits"""
    lib = ntscsim.lib()
    lo, hi = 1, 1 << 22
    assert lib.ntscsim_debug_fast_plane_ok(lo, w, h, hs_mode) == 1 and lib.ntscsim_debug_fast_plane_ok(hi, w, h, hs_mode) == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if lib.ntscsim_debug_fast_plane_ok(mid, w, h, hs_mode):
            lo = mid
        else:
            hi = mid
    return lo


def test_the_plane_of_the_whole_call_decides_at_720x486():
    """The rule reads the CALL's Rpad: a set keeps its hand-tuned forms up to the last field count the plane rule admits
    for the set's head-switch range, and takes the generic forms of its class one field past it -- however few fields
    the set's own group would hold."""
    w, h = 720, 486
    flags = {c[0]: c[1] for c in cases.CASES}
    n0, n1, n2 = (last_ok(w, h, m) for m in (0, 1, 2))
    assert n2 < n1 < n0
    # (Rpad moves in steps of 64 rows: the first count whose plane is refused may lie a few fields further on)
    def first_bad(n, m):
        while ntscsim.lib().ntscsim_debug_fast_plane_ok(n, w, h, m):
            n += 1
        return n
    default, vhs = L.make_params([]), L.make_params(["-vhs"])
    pal, sv, catv_vhs = L.make_params(flags["vhs_pal"]), L.make_params(flags["vhs_svideo"]), L.make_params(flags["catv4_vhs"])
    # no head switching: range 0
    assert form_of(default, w, h, n0) == (ENC_FAST, DEC_TV)
    assert form_of(default, w, h, first_bad(n0, 0)) == (ENC_GENERIC, DEC_GEN_TV)
    # -vhs: displacements within w / 10, range 1
    assert form_of(vhs, w, h, n1) == (ENC_FAST, DEC_VHS)
    assert form_of(vhs, w, h, first_bad(n1, 1)) == (ENC_GENERIC, DEC_GEN_VCR)
    # PAL's switching point: any displacement, range 2
    assert form_of(pal, w, h, n2) == (ENC_FAST, DEC_VHS_WR)
    assert form_of(pal, w, h, first_bad(n2, 2)) == (ENC_GENERIC, DEC_GEN_VCR)
    # forms whose loads wrap around whatever the set's displacement: the decoder leaves at the range-2 threshold, the
    # encoder stays to the set's own
    for p, dec, gen in ((sv, DEC_SV, DEC_GEN_SV), (catv_vhs, DEC_BK_VHS, DEC_GEN_VCR)):
        enc = form_of(p, w, h, 4)[0]
        assert enc in (ENC_FAST, ENC_FAST_PRE)
        assert form_of(p, w, h, n2) == (enc, dec)
        assert form_of(p, w, h, first_bad(n2, 2)) == (enc, gen)
        assert form_of(p, w, h, n1) == (enc, gen)
        assert form_of(p, w, h, first_bad(n1, 1)) == (ENC_GENERIC, gen)
