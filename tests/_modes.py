"""ctypes bindings of oracle/ntsc_modes_oracle.h (the mode model: exact64 / fast32 / real64 / real32), the inputs and the
case list shared by tests/test_modes_oracle.py (CPU), tests/test_float_model_gpu.py, tests/test_fast32_model_gpu.py, the
FAST32 form table (tests/_fast32_forms.py and its two test files) and tools/float_model_err.py.  Test infrastructure only;
no GPU import."""
import ctypes as C

import numpy as np

import _libs as L

# the kernels' constant in front of the final truncation (csrc/ntsc_float.hip: NTSC_FP_LUMA_BIAS_*), units of the
# 256-scaled signal
LUMA_BIAS_VHS = -2.25
LUMA_BIAS_DEF = -0.875


class ModesPlanes(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("composite", "final_y", "final_i", "final_q", "v")]


_bound = False


def lib():
    global _bound
    o = L.oracle()
    if not _bound:
        common = [C.POINTER(L.Params), C.POINTER(L.OracleRng), L._u8p, C.c_int, C.c_int, C.c_int, L._u8p, C.c_int,
                  C.c_int, C.c_int, C.c_uint, C.c_uint64]
        for name in ("ntsc_modes_exact64", "ntsc_modes_fast32"):
            f = getattr(o, name)
            f.argtypes = common + [C.POINTER(L.OracleTaps)]
            f.restype = C.c_int
        for name in ("ntsc_modes_real64", "ntsc_modes_real32"):
            f = getattr(o, name)
            f.argtypes = common + [C.c_double, C.POINTER(ModesPlanes)]
            f.restype = C.c_int
        _bound = True
    return o


def luma_bias(params):
    return LUMA_BIAS_VHS if params.emulating_vhs else LUMA_BIAS_DEF


class ModelStream:
    """One flavour of the model driven like the field loop: one rand() stream across calls.
    flavour: "exact64", "fast32" (int32 taps, as L.OracleStream) or "real64", "real32" (planes of the flavour's type)."""

    def __init__(self, params, flavour):
        self.p, self.flavour = params, flavour
        self.real = flavour.startswith("real")
        self.dtype = np.float32 if flavour.endswith("32") else np.float64
        self.fn = getattr(lib(), "ntsc_modes_" + flavour)
        self.g = L.OracleRng()
        L.oracle().ntsc_oracle_rng_seed(C.byref(self.g), 1)

    @property
    def rng_pos(self):
        return int(self.g.count)

    def field(self, dst, src, field, fieldno, interlaced=0, tff=0, taps=None, bias=None):
        """real flavours: returns {"composite", "final_y", "final_i", "final_q": [L, W], "v": [L, W, 3] (r, g, b)};
        the others: the requested int32 taps as [L, W]."""
        h, w = src.shape[:2]
        assert dst.shape == src.shape and src.flags.c_contiguous and dst.flags.c_contiguous
        rows = L.field_rows(h, field)
        head = [C.byref(self.p), C.byref(self.g), L._ptr(src), w * 4, interlaced, tff, L._ptr(dst), w * 4, w, h, field, fieldno]
        if self.real:
            out = {n: np.zeros((rows, w, 3) if n == "v" else (rows, w), self.dtype) for n, _ in ModesPlanes._fields_}
            pl = ModesPlanes()
            for n, a in out.items():
                setattr(pl, n, a.ctypes.data)
            rc = self.fn(*head, luma_bias(self.p) if bias is None else bias, C.byref(pl))
            assert rc == 0
            return out
        t, keep = None, {}
        if taps:
            t = L.OracleTaps()
            for name in taps:
                keep[name] = np.zeros(rows * w, np.int32)
                setattr(t, name, keep[name].ctypes.data_as(C.POINTER(C.c_int32)))
        rc = self.fn(*head, C.byref(t) if t is not None else None)
        assert rc == 0
        return {k: v.reshape(rows, w) for k, v in keep.items()}


# ---------------------------------------------------------------------------------------------- inputs
def ramp(w, h):
    """the ramp of tests/test_gpu_fast_mode.py"""
    x = np.arange(w)[None, :]
    y = np.arange(h)[:, None]
    fr = np.zeros((h, w, 4), np.uint8)
    fr[..., 0] = x * 255 // max(1, w - 1)
    fr[..., 1] = y * 255 // max(1, h - 1)
    fr[..., 2] = (x + y) * 255 // max(1, w + h - 2)
    return fr


def saturating(w, h):
    """blocks of pure white and black, 5 pixels by 3 rows (no multiple of a kernel's 4-pixel step): with -noise 100 both
    clamps of the output are hit"""
    x = np.arange(w)[None, :] // 5
    y = np.arange(h)[:, None] // 3
    fr = np.zeros((h, w, 4), np.uint8)
    fr[..., :3] = (((x + y) & 1) * 255).astype(np.uint8)[..., None]
    return fr


def decay(w, h):
    """rows whose first W/8 pixels are saturated blue with a little red and whose last W/8 are green, black between: the
    chroma states fall towards zero over the black run (hundreds of samples at W = 720) before colour returns -- long
    decays, where a kernel that flushed small states to zero would part from the model.  (Whether the float states reach
    the subnormal range at W = 720 has not been measured.)  Every third row is all 0, every fifth all 255 (a row that is
    both is 255)."""
    e = max(1, w // 8)
    fr = np.zeros((h, w, 4), np.uint8)
    fr[:, :e, 0], fr[:, :e, 2] = 255, 24          # memory order B, G, R
    fr[:, w - e:, 1] = 255
    fr[0::3, :, :3] = 0
    fr[0::5, :, :3] = 255
    return fr


def sources(kind, w, h):
    """the source frames of a case: field k reads frame k % len"""
    if kind == "mixed":
        return [L.noise_frame(w, h, 0x51 + w + h), L.bars(w, h, 3), ramp(w, h)]
    if kind == "saturating":
        return [saturating(w, h)]
    if kind == "decay":
        return [decay(w, h)]
    if kind == "noise":
        return [L.noise_frame(w, h, 0x51 + w + h), L.noise_frame(w, h, 0x52 + w + h)]
    raise ValueError(kind)


def jobs(n, nsrc):
    """(src index, field, fieldno) per output field: parities alternate from field 1, fieldno advances"""
    return [(k % nsrc, (k & 1) ^ 1, k) for k in range(n)]


# ---------------------------------------------------------------------------------------------- FLOAT cases
# (id, flags, W, H, fields, source kind, form, extra)
#   form   "fp"      the all-float kernels must run (k_encode_fp + k_decode_fp*): checked against real64
#          "fast32"  the switch set / geometry is outside the float forms: the FAST32 kernels must run, checked for
#                    EQUALITY with the fast32 flavour
#          "refused" the C ABI must refuse the geometry (NTSCSIM_E_SIZE)
#   extra  {"interlaced": 1, "tff": 1} descriptor flags; {"pad": n} device rows of n pixels; {"decoder": name} the decoder
#          form the case is FOR (asserted: a case list that drifts from the dispatcher's rule fails)
VHS = ["-vhs"]
LP = ["-vhs", "-vhs-speed", "lp"]
EP = ["-vhs", "-vhs-speed", "ep"]
SAT = ["-noise", "100"]


def _hs_phase(w, hx, lines=262.5):
    """-vhs-head-switching-phase that puts the switch at sample hx of the 1.1 W window (row 0 of the phase)"""
    tw = w + w // 10
    return "%.9f" % ((hx + 0.5) / (lines * tw))


def _float_cases():
    out = []

    def add(name, flags, w, h, n=6, kind="mixed", form="fp", **extra):
        out.append((name, list(flags), w, h, n, kind, form, extra))

    # encoder steady loop: 4 + 16 <= W.  none / one chunk / one + remainder / two / two + remainder
    for w in (16, 20, 24, 36, 40):
        add("enc_w%d" % w, VHS, w, 10)
    # The -vhs decoder has two forms with different loop conditions; the number of fields of a launch selects the form
    # (<= 128: k_decode_fp2, more: k_decode_fp<true>), so each condition gets its own widths AND its own batch length.
    # Widths are multiples of 4 (16-byte rows): below / first width inside / above.
    #
    # (a) k_decode_fp<true>, steady(): entered at t = SKT = 15 + d when SKT + 4 <= W - max(d - 7, 0):
    #     SP (d = 9) from W >= 30, LP (12) from 36, EP (14) from 40.  130 fields -> the one-wave form, asserted by name;
    #     its instantiations steady<true, DPH>, DPH = (SKT - 7) & 3 = 1 / 0 / 2 for SP / LP / EP, all run
    for spd, fl, ws in (("sp", VHS, (28, 32, 36)), ("lp", LP, (32, 36, 40)), ("ep", EP, (36, 40, 44))):
        for w in ws:
            add("dec1_%s_w%d" % (spd, w), fl, w, 10, 130, decoder="k_decode_fp<true>")
    # (b) k_decode_fp2, VCR role, vcr_steady(): entered at t = 7 + d when 7 + d + 4 <= W - max(d - 7, 0):
    #     SP from W >= 22, LP from 28, EP from 32.  Below it the role runs vcr_edge() alone from fill to tail.
    #     (TV role: its loop starts at u = 8 and needs 8 + 4 <= W -- always entered, the ABI takes no W < 16; its 32-slot
    #     ring of composite samples wraps for W > 32: 28 / 32 / 36 lie on either side)
    for spd, fl, ws in (("sp", VHS, (20, 24, 28)), ("lp", LP, (24, 28, 32)), ("ep", EP, (28, 32, 36))):
        for w in ws:
            add("dec2_%s_w%d" % (spd, w), fl, w, 10, decoder="k_decode_fp2")
    # (c) the widths of (a) as short launches too: k_decode_fp2 well inside its loops, ring wrapped
    for w in (32, 36):
        add("dec2_sp_w%d" % w, VHS, w, 10, decoder="k_decode_fp2")
    for w in (36, 40):
        add("dec2_lp_w%d" % w, LP, w, 10, decoder="k_decode_fp2")
    for w in (40, 44):
        add("dec2_ep_w%d" % w, EP, w, 10, decoder="k_decode_fp2")
    # default preset: SKT = 8, d = 0: enters at W >= 12 -- but ntscsim_fields_device() takes no width below 16, so that
    # loop's "not entered" side cannot be reached: 8 and 12 must be REFUSED (form "refused"), 16 and 20 run
    for w in (8, 12):
        add("dec_def_w%d" % w, [], w, 10, form="refused")
    for w in (16, 20):
        add("dec_def_w%d" % w, [], w, 10)
    # a 16-pixel store burst completes (64) / a partial one is left to the guarded steps (68): in the TV role of
    # k_decode_fp2 (6 fields), in steady() of k_decode_fp<true> (130 fields) and in k_decode_fp<false>
    for w in (64, 68):
        add("burst_sp_w%d" % w, VHS, w, 10, decoder="k_decode_fp2")
        add("burst1_sp_w%d" % w, VHS, w, 10, 130, decoder="k_decode_fp<true>")
        add("burst_def_w%d" % w, [], w, 10)
    # saturating input per family (both clamps)
    add("sat_sp_w40", VHS + SAT, 40, 10, 2, "saturating")
    add("sat_sp_w68", VHS + SAT, 68, 10, 2, "saturating")
    add("sat_ep_w44", EP + SAT, 44, 10, 2, "saturating")
    add("sat_def_w16", SAT, 16, 10, 2, "saturating")
    add("sat_def_w68", SAT, 68, 10, 2, "saturating")
    add("sat_rows_h127", VHS + SAT, 40, 127, 2, "saturating")
    add("sat_rows_h128_def", SAT, 40, 128, 2, "saturating")
    add("sat_hs_disp4", VHS + SAT + ["-vhs-head-switching-point", "0.105", "-vhs-head-switching-phase", _hs_phase(40, 4)],
        40, 32, 2, "saturating")
    add("sat1_sp_w36", VHS + SAT, 36, 10, 130, "saturating", decoder="k_decode_fp<true>")
    # row packing: 63-row workgroups (lane 0 = halo) cutting through fields, fields cutting through wavefronts
    # (4 fields where the issue's list says 2: the third source frame, the ramp, is field 2's; fields 0 and 1 are the
    #  two-field geometry it names, and the wavefront boundaries of fields 2 and 3 fall elsewhere again)
    add("rows_h100_n4", VHS, 40, 100, 4)
    for h in (126, 127, 128, 130):
        add("rows_h%d" % h, VHS, 40, h, 4)
    add("rows_h9", VHS, 40, 9)
    add("rows_h9_def", [], 20, 9)
    add("rows_h100_noblend", VHS + ["-vhs-chroma-vblend", "0"], 40, 100, 4)
    add("rows_h128_def", [], 40, 128, 4)
    # PAL: no vertical blend; the default switching phase is displaced by 0.18 of the window (> W/10) -> placed at -1 %
    add("pal_h100", ["-tvstd", "pal", "-vhs", "-vhs-head-switching-phase", "%.9f" % (0.99 / 312.5)], 40, 100, 4)
    add("pal_default_phase", ["-tvstd", "pal", "-vhs"], 40, 20, 4, form="fast32")
    # descriptor flags
    add("interlaced_tff", VHS, 40, 18, 4, interlaced=1, tff=1)
    add("interlaced_bff_def", [], 40, 18, 4, interlaced=1, tff=0)
    # row constants
    for w in (28, 40):
        add("dropout_w%d" % w, VHS + ["-chroma-dropout", "30000"], w, 18)
    add("dropout_def_w16", ["-chroma-dropout", "30000"], 16, 18)
    add("dropout_def_w40", ["-chroma-dropout", "30000"], 40, 18)
    add("phase_noise_max", VHS + ["-chroma-phase-noise", "4096"], 40, 18)
    add("hs_point08_360x244", VHS + ["-vhs-head-switching-point", "0.8"], 360, 244, 2, "noise")
    # (point 0.8 is line 210 of the field raster = frame row 376 + field: with 244 rows the switch row itself lies below
    #  the picture and the case covers the per-row shift table with nothing to shift; the next three put it inside)
    # the switch inside a small frame (line 27 of the field raster -> frame row 10 + field)
    add("hs_inside", VHS + ["-vhs-head-switching-point", "0.105"], 40, 32, 4)
    # displacement just inside / just outside W/10 = 4 at W = 40
    add("hs_disp4", VHS + ["-vhs-head-switching-point", "0.105", "-vhs-head-switching-phase", _hs_phase(40, 4)], 40, 32, 4)
    add("hs_disp5", VHS + ["-vhs-head-switching-point", "0.105", "-vhs-head-switching-phase", _hs_phase(40, 5)], 40, 32, 4,
        form="fast32")
    # an odd width on padded, 16-byte-aligned rows: the eligibility check looks at pointers and linesizes only, so the
    # float forms run it (pad = pixels per row of the device buffers)
    add("odd_w33_padded", VHS, 33, 17, 4, pad=36)
    add("odd_w21_padded_def", [], 21, 9, 4, pad=24)
    # rows that are not 16-byte aligned: the FAST32 forms
    add("odd_w33", VHS, 33, 17, 4, form="fast32")
    return out


FLOAT_CASES = _float_cases()
# the long batch: more than 128 fields per launch take k_decode_fp<true>, the same jobs in launches of <= 128 k_decode_fp2
LONG_BATCH = ("long_batch", VHS + ["-vhs-head-switching-point", "0.105"], 40, 18, 130, "mixed")
