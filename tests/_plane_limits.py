"""The case table of tests/test_plane_limits_gpu.py and tests/test_plane_limits_host.py: launches of the exact BGRA
field path whose transposed composite plane crosses the sizes at which the launcher changes kernels
(fast_plane_ok(), csrc/ntscsim_hip.hip) or refuses the call (prepare_records()).

Every field count is derived from ntscsim_debug_fast_plane_ok(n, W, H, mode) and from the launcher's
Rpad = ceil(n * Lslot / 64) * 64 + 64; none is typed in.  The GPU half runs the launches, the host half shows that
the table crosses what it claims."""
import _libs as L
import ntscsim
from ntscsim import _capi

W, H = 720, 486                     # the geometry of every big case
S = 7                               # distinct source frames (odd: every source feeds fields of both parities)
CHUNK = 600                         # fields of one small-launch twin (the bench clip's length)
FILL = 0x55
GIB = 1 << 30

HS_POS = ["-vhs-head-switching-point", "0.105", "-vhs-head-switching-phase", "0.0012"]     # displaced to the right
HS_NEG = ["-vhs-head-switching-point", "0.105", "-vhs-head-switching-phase", "0.002"]      # ... and to the left
GHOST_TAPS = ((12, 64), (31, -32))  # delays <= 63: folded into the hand-tuned encoder where that one runs


# ---- the launcher's arithmetic ---------------------------------------------------------------------------------
def lslot(h):
    return (h + 1) // 2


def rows(n, h):
    return n * lslot(h)


def rpad(n, h):
    return (rows(n, h) + 63) // 64 * 64 + 64


def plane_bytes(n, w, h):
    return rpad(n, h) * w * 4


def plane_ok(n, w, h, mode):
    return bool(L.product().ntscsim_debug_fast_plane_ok(int(n), int(w), int(h), int(mode)))


def n_fit(mode, w=W, h=H):
    """The largest field count whose plane the predicate admits for head-switch mode 0 | 1 | 2."""
    lo, hi = 1, 2
    assert plane_ok(lo, w, h, mode)
    while plane_ok(hi, w, h, mode):
        lo, hi = hi, hi * 2
    while hi - lo > 1:              # plane_ok(lo) and not plane_ok(hi)
        mid = (lo + hi) // 2
        if plane_ok(mid, w, h, mode):
            lo = mid
        else:
            hi = mid
    return lo


def n_over(w=W, h=H):
    """The smallest field count whose plane is at least 1.05 * 2^32 bytes: an index cut to 32 bits would alias at
    least 0.05 * 2^32 / (Rpad * 4) > 30 whole columns, not just the padding rows."""
    want = -(-(105 * (1 << 32)) // 100)
    n = want // (lslot(h) * w * 4) - 2
    while plane_bytes(n, w, h) < want:
        n += 1
    return n


def n_elems_refused(w=W, h=H):
    """The smallest count with Rpad * W > 2^31 elements (NTSCSIM_E_SIZE); the one before it is the largest accepted."""
    n = (1 << 31) // (w * lslot(h)) - 2
    while rpad(n, h) * w <= (1 << 31):
        n += 1
    return n


ROWS_REFUSED = (16, 16384, (1 << 30) // lslot(16384) + 1)       # (W, H, n): R = 2^30 + Lslot rows


def head_switch_shifts(p, w):
    """head_switch_is_small()'s arithmetic (csrc/ntscsim_hip.hip): the initial displacement, in samples, at the two
    ends of the phase-noise range, or None where the ends fall into different rows."""
    import math
    tw = w + w // 10
    t = tw * (262.5 if p.tv_standard == 0 else 312.5)
    pn = abs(p.vhs_head_switching_phase_noise)
    out = []
    for a in (p.vhs_head_switching_phase - pn, p.vhs_head_switching_phase + pn):
        if a < 0:
            return None
        pp = int((a - math.trunc(a)) * t)
        hx = pp % tw
        out.append(hx - tw if hx >= tw // 2 else hx)
    return out


def hs_mode(p, w):
    """0 no head switching, 1 displacement <= W/10, 2 anything else: the launcher's choice of threshold."""
    if not p.vhs_head_switching:
        return 0
    sh = head_switch_shifts(p, w)
    tw = w + w // 10
    if sh is None or (sh[0] < 0) != (sh[1] < 0):
        return 2
    return 1 if max(abs(s) for s in sh) <= tw - w else 2


# ---- the table -------------------------------------------------------------------------------------------------
ENC_FAST, ENC_XI, ENC_GEN = "k_encode_fast<double>", "k_encode_fast_xi<double>", "k_encode<8u,double>"
DEC_TV, DEC_VHS, DEC_WR = "k_decode_fast<false,double>", "k_decode_fast<true,double>", "k_decode_fast<true,double,true>"
GEN_TV, GEN_VHS, GEN_VHS_RT = "k_decode<false,false,0u,double>", "k_decode<true,true,6u,double>", "k_decode<true,true,1u,double>"


class Case:
    """id, switches, which threshold of the predicate it sits at (mode), the count as (mode, +0 | +1) or "over", and
    the forms ntscsim_debug_last_kernels() must name, setup kernels aside."""

    def __init__(self, cid, flags, mode, at, forms, debug=0, ghost=(), sim_mode=_capi.MODE_EXACT, planes=1):
        self.id, self.flags, self.mode, self.at, self.forms = cid, list(flags), mode, at, list(forms)
        self.debug, self.ghost, self.sim_mode, self.planes = debug, tuple(ghost), sim_mode, planes
        self.w, self.h = W, H

    @property
    def n(self):
        return n_over(self.w, self.h) if self.at == "over" else n_fit(self.mode, self.w, self.h) + self.at

    def params(self):
        p = L.make_params(self.flags)
        p.ghost_taps = len(self.ghost)
        for k, (d, g) in enumerate(self.ghost):
            p.ghost_delay[k], p.ghost_gain[k] = d, g
        return p

    def key(self):
        return (tuple(self.flags), self.ghost, self.w, self.h)

    def peak_bytes(self):
        """Device memory of the test at its peak: composite planes, destination(s) with the guard frame, the scratch
        clip of the small-launch twins, sources, and the per-row tables (31 + 1 ints of luma state and 31 + 2 of
        chroma state per padded row, three per-row tables, 2 KiB of tails per 63 rows)."""
        n, w, h = self.n, self.w, self.h
        frame = w * h * 4
        dst = ((n + 1) // 2 + 1) * frame
        tables = rpad(n, h) * 4 * (32 + 33) + rows(n, h) * 4 * 3 + (rows(n, h) + 62) // 63 * 32 * 64 * 4
        float_too = self.sim_mode == _capi.MODE_FLOAT         # case 8 keeps the exact destination beside the FLOAT one
        return self.planes * plane_bytes(n, w, h) + dst * (2 if float_too else 1) + (CHUNK // 2) * frame + S * frame + tables


def _cases():
    vhs = ["-vhs"]
    xi = ["-vhs", "-comp-phase", "90"]
    fo = ["-vhs", "-out-composite-lowpass-lite", "0"]
    FL = _capi.MODE_FLOAT
    c = [
        Case("1-default-fit", [], 0, 0, [ENC_FAST, DEC_TV]),
        Case("2-default-fit+1", [], 0, 1, [ENC_GEN, GEN_TV]),
        Case("2-default-over", [], 0, "over", [ENC_GEN, GEN_TV]),
        Case("3-vhs-fit", vhs, 1, 0, [ENC_FAST, DEC_VHS]),
        Case("3-vhs-fit-two-launch", vhs, 1, 0, [ENC_FAST, "k_vcr_front<double>", DEC_TV], debug=2, planes=2),
        Case("4-vhs-fit+1", vhs, 1, 1, [ENC_GEN, GEN_VHS]),
        Case("4-vhs-over", vhs, 1, "over", [ENC_GEN, GEN_VHS]),
        Case("5-wrap-right-fit", vhs + HS_POS, 2, 0, [ENC_FAST, DEC_WR]),
        Case("5-wrap-left-fit", vhs + HS_NEG, 2, 0, [ENC_FAST, DEC_WR]),
        Case("6-wrap-right-fit+1", vhs + HS_POS, 2, 1, [ENC_GEN, GEN_VHS]),
        Case("6-wrap-left-fit+1", vhs + HS_NEG, 2, 1, [ENC_GEN, GEN_VHS]),
        # the xi and fo decoders test the mode-2 threshold whatever the displacement; past it the encoder, which
        # tests mode 1 for these small displacements, is still the hand-tuned one
        Case("7-xi-fit", xi, 2, 0, [ENC_XI, "k_decode_fast_xi<double>"]),
        Case("7-xi-fit+1", xi, 2, 1, [ENC_XI, GEN_VHS]),
        Case("7-fo-fit", fo, 2, 0, [ENC_FAST, "k_decode_fast_fo<double>"]),
        Case("7-fo-fit+1", fo, 2, 1, [ENC_FAST, GEN_VHS_RT]),
        Case("8-float-fit", vhs, 1, 0, ["k_encode_fp", "k_decode_fp<true>"], sim_mode=FL),
        Case("8-float-fit+1", vhs, 1, 1, ["k_encode<8u,float>", "k_decode<true,true,6u,float>"], sim_mode=FL),
        Case("9-ghost-fit", [], 0, 0, ["k_encode_fast_gh<double,2>", DEC_TV], ghost=GHOST_TAPS),
        Case("9-ghost-fit+1", [], 0, 1, [ENC_GEN, "k_ghost", GEN_TV], ghost=GHOST_TAPS, planes=2),
    ]
    return c


CASES = _cases()
# case 8 pins the exact output of its descriptors to the oracle first: the forms of that launch
EXACT_FORMS_OF_FLOAT = {"8-float-fit": [ENC_FAST, DEC_VHS], "8-float-fit+1": [ENC_GEN, GEN_VHS]}


def case(cid):
    return [c for c in CASES if c.id == cid][0]


# ---- descriptors, positions, samples ---------------------------------------------------------------------------
def jobs(n, first=0, dst_base=None):
    """Field k: (source k % S, destination frame k // 2, field (k & 1) ^ 1, fieldno k).  The two fields of a pair
    share one destination frame.  dst_base: the destination index of field `first` (default first // 2)."""
    base = first // 2 if dst_base is None else dst_base
    return [(k % S, k // 2 - first // 2 + base, (k & 1) ^ 1, k) for k in range(first, first + n)]


class Positions:
    """shard.rng_pos_of_field with the two draw counts looked up once."""

    def __init__(self, p, w, h):
        self.c1 = ntscsim.calls_per_field(p, w, h, 1)       # even field numbers take field 1
        self.c0 = ntscsim.calls_per_field(p, w, h, 0)

    def __call__(self, k):
        return (k + 1) // 2 * self.c1 + k // 2 * self.c0


def sampled_fields(n, h):
    """At least 8 distinct fields, fixed by the count: the first, the last, the middle one, the field holding the
    last row of the last full 64-row wavefront, the field holding the first row of the last 63-row workgroup, and
    fields spread by a fixed stride of n // 7 until there are eight."""
    ls, r = lslot(h), rows(n, h)
    named = [0, n - 1, n // 2, (r // 64 * 64 - 1) // ls, ((r + 62) // 63 - 1) * 63 // ls]
    out = []
    for k in named + [j * (n // 7) + 1 for j in range(1, 7)]:
        if 0 <= k < n and k not in out:
            out.append(k)
        if len(out) >= 8 and all(x in out for x in named):
            break
    return named, out


_sources = {}


def sources(w, h):
    """S frames, noise and bars in turn (numpy [S, h, w, 4]); made once and never written."""
    import numpy as np
    if (w, h) not in _sources:
        a = np.stack([L.noise_frame(w, h, 0x5150 + j) if j % 2 == 0 else L.bars(w, h, 3 * j) for j in range(S)])
        a.setflags(write=False)
        _sources[(w, h)] = a
    return _sources[(w, h)]
