"""ntscsim_field422() / ntscsim_submit422() across a RE-MAKE of the engine's device rings in mid-stream (h422_release_rings,
csrc/ntscsim_host422.hip): a ctx that goes from the synchronous call's two slots to a submit's `nslots`, a
ntscsim_submit422_configure() between two iterations, a taller source, another frame size on the same caller memory -- and
the neighbours of those: synchronous calls on rings a submit has grown (they chain on the device), SUBMIT_SAME_SRC right
behind a re-make, ntscsim_host_unpin(ctx, NULL) between two chained iterations.

Tight rows (linesize == width, width >= 128) are what makes a re-make visible: the two bytes behind each row are chained on
the device frame that the previous iteration of the OTHER field wrote (H422Writers, csrc/engine_host.hpp), and device frames
do not survive a re-make.  Every scenario is a script of steps that runs twice: through the oracle's in-order loop and through
the host API on byte-identical buffers; whole buffers are compared (the frame's memory with every byte behind the rows, every
encoder frame, the rand() position), tolerance zero.  The stats say that the iterations behind the transition were still
batched: neither hiding the chain behind the one-at-a-time path nor dropping it would pass."""

import numpy as np
import pytest

import _libs as L
from ntscsim import _capi
from test_host422 import (F_420, F_SECOND, OUT_BOB420, OUT_BOB422, Ctx, enc_frame, oracle_iteration, paged_noise,
                          random_padding, same_frames, same_out)

pytestmark = pytest.mark.gpu


class FrameOn(L.Yuv422):
    """A YUV422P frame laid over memory that exists already, at its base address: what a caller does that reuses one
    allocation for frames of another size.  `buf` stays the WHOLE memory, so comparisons cover every byte of it."""

    def __init__(self, buf, w, h, pad=0):
        self.w, self.h = w, h
        self.ls = [w + pad, w // 2 + pad, w // 2 + pad]
        sizes = [self.ls[i] * h for i in range(3)]
        assert sum(sizes) <= buf.size, "the frame does not fit into the caller's memory"
        self.buf = buf
        self.off = [0, sizes[0], sizes[0] + sizes[1]]


# ---- steps of a script -------------------------------------------------------------------------------------------------------
def field(n=1):
    """n iterations through ntscsim_field422()"""
    return [("field", None)] * n


def submit(n=1, flags=None):
    """n iterations through ntscsim_submit422(); flags None: SUBMIT_SAME_SRC for the second field of a source, else 0"""
    return [("submit", flags)] * n


def wait(k=None):
    """ntscsim_wait() for iteration k of the script (negative: counted from the last one submitted), None: everything"""
    return [("wait", k)]


def configure(depth, slots):
    return [("configure", depth, slots)]


def unpin():
    """ntscsim_host_unpin(ctx, NULL)"""
    return [("unpin",)]


def src_height(sh):
    """the next source (and those behind it) has sh rows"""
    return [("src_height", sh)]


def frame_is(w, h, pad=0):
    """the frame is now w x h, at the base address it always had"""
    return [("frame", w, h, pad)]


def mark():
    """note the engine's stats and the number of iterations so far"""
    return [("mark",)]


def run_script(p, steps, w, h, pad=0, out_mode=OUT_BOB420, src_flags=0, paged=False, declare=False, seed=5):
    """Runs `steps` through the oracle's in-order loop and through the host API on byte-identical buffers and asserts
    whole-buffer equality of everything the loop touches, as test_host422.run_loop does.  Iteration vf (0, 1, ...) takes
    field (vf & 1) ^ 1 of source vf // 2; its ticket is vf + 1, whichever call made it.  Returns [(iterations, stats), ...]:
    one entry per mark() and one for the end."""
    def play(ctx):
        """ctx None: the oracle"""
        first = paged_noise(w, h, seed, pad) if paged else L.yuv_noise(w, h, seed, pad)
        random_padding(first, seed + 1)
        if ctx is not None and declare:
            assert ctx.lib.ntscsim_host_pin(ctx.h, first.buf.ctypes.data, first.buf.nbytes) == 0
        o = L.TocompOracleStream(p, oob=L.OOB_PLANE) if ctx is None else None
        fr, sh, src = first, h, None
        outs, marks, vf = [], [], 0
        for st in steps:
            if st[0] in ("field", "submit"):
                f_ = (vf & 1) ^ 1
                sub = vf & 1
                if not sub:
                    src = L.yuv_noise(fr.w, sh, 100 + vf // 2)
                fl = src_flags | (F_SECOND if sub else 0)
                eo = enc_frame(fr.w, fr.h, out_mode, fill=7)
                outs.append(eo)
                if ctx is None:
                    oracle_iteration(o, p, fr, src, f_, vf, fl, None, eo, out_mode, f_)
                else:
                    it = ctx.loop(fr, src, f_, vf, fl, None, eo, out_mode, f_, sh=sh)
                    if st[0] == "field":
                        ctx.field(it)
                    else:
                        sf = st[1] if st[1] is not None else (_capi.SUBMIT_SAME_SRC if sub else 0)
                        assert ctx.submit(it, sf) == vf + 1
                vf += 1
            elif st[0] == "src_height":
                assert not (vf & 1), "a source changes between two frames, not between its fields"
                sh = st[1]
            elif st[0] == "frame":
                assert not (vf & 1)
                if ctx is not None:
                    ctx.wait()              # (the caller looks at its memory anew: nothing may be in flight)
                fr = FrameOn(first.buf, st[1], st[2], st[3])
                sh = st[2]
            elif ctx is None:
                continue
            elif st[0] == "wait":
                k = st[1]
                ctx.wait(_capi.TICKET_ALL if k is None else (k if k >= 0 else vf + k) + 1)
            elif st[0] == "configure":
                assert ctx.lib.ntscsim_submit422_configure(ctx.h, st[1], st[2]) == 0
            elif st[0] == "unpin":
                ctx.unpin()
            elif st[0] == "mark":
                marks.append((vf, ctx.stats()))
            else:
                raise ValueError(st)
        if ctx is not None:
            ctx.wait()
            marks.append((vf, ctx.stats()))
        return first, fr, outs, (o.rng_pos if ctx is None else ctx.rng_pos), marks

    first_o, last_o, outs_o, pos_o, _ = play(None)
    ctx = Ctx(p)
    try:
        first_g, last_g, outs_g, pos_g, marks = play(ctx)
        if declare or paged:
            ctx.unpin()
    finally:
        ctx.close()
    assert pos_g == pos_o
    assert first_g.buf.size == first_o.buf.size
    same_frames(last_g, last_o, "frame")            # (.buf is the caller's whole memory, whatever frame lies over it now)
    assert len(outs_g) == len(outs_o)
    for i, (a, b) in enumerate(zip(outs_g, outs_o)):
        same_out(a, b, a.h, out_mode, "encoder frame %d" % i, tight=pad < 2)
        assert np.array_equal(a.buf, b.buf), "encoder frame %d: bytes outside its rows" % i
    return marks


def still_batched(marks, serial_before=0):
    """every iteration behind the (last) mark ran batched, none one at a time"""
    (n0, s0), (n1, s1) = marks[-2], marks[-1]
    assert n1 > n0
    assert s1[3] - s0[3] == n1 - n0 and s1[4] == s0[4] == serial_before, (marks[-2], marks[-1])
    assert s1[0] == n1


# the shapes of the tight scenarios: 128 is the narrowest width that chains
SHAPES = [(["-vhs"], 256, 36, OUT_BOB420), (["-vhs", "-vhs-speed", "ep"], 128, 35, OUT_BOB422)]
SHAPE_IDS = ["vhs-256x36", "ep-128x35"]


def params_of(flags, w, h):
    return L.make_params_tocomp(flags + ["-width", str(w)], output_height=h)


def scenario_a():
    """sync then async: the rings go from the synchronous call's 2 slots to nslots"""
    return configure(8, 0) + field(2) + mark() + submit(12)


def scenario_c():
    """more slots in mid-stream"""
    return configure(2, 0) + submit(10) + mark() + configure(8, 0) + submit(10)


def scenario_d():
    """fewer slots in mid-stream: live device frames reach the high twenties of 32, then 6 slots"""
    return configure(8, 32) + submit(30) + mark() + configure(2, 6) + submit(8)


@pytest.mark.parametrize("flags,w,h,out_mode", SHAPES, ids=SHAPE_IDS)
def test_a_synchronous_calls_then_submits(flags, w, h, out_mode):
    """Two ntscsim_field422() calls on a fresh ctx (a ring of two), then submits at depth 8: the first submit re-makes the
    rings with 32 slots, and its tight rows must take the caller's bytes, not slot 0 or 1 of the new allocation."""
    still_batched(run_script(params_of(flags, w, h), scenario_a(), w, h, 0, out_mode))


@pytest.mark.parametrize("flags,w,h,out_mode", SHAPES, ids=SHAPE_IDS)
def test_b_submits_then_synchronous_calls_that_chain(flags, w, h, out_mode):
    """Six submits at depth 8, a wait, then ntscsim_field422() for ten iterations: the rings stay at 32 slots, so the
    synchronous calls chain on the device (with a ring of two they never do); then submits again."""
    steps = configure(8, 0) + submit(6) + wait() + mark() + field(10) + submit(8)
    still_batched(run_script(params_of(flags, w, h), steps, w, h, 0, out_mode))


@pytest.mark.parametrize("flags,w,h,out_mode", SHAPES, ids=SHAPE_IDS)
def test_c_configure_to_more_slots_in_mid_stream(flags, w, h, out_mode):
    still_batched(run_script(params_of(flags, w, h), scenario_c(), w, h, 0, out_mode))


@pytest.mark.parametrize("flags,w,h,out_mode", SHAPES, ids=SHAPE_IDS)
def test_d_configure_to_fewer_slots_in_mid_stream(flags, w, h, out_mode):
    """The writer table of a 32-slot ring names slots in the high twenties; the rings re-made with 6 slots have no such
    slot (tests/engine_host_check.cpp walks the same case without a GPU)."""
    still_batched(run_script(params_of(flags, w, h), scenario_d(), w, h, 0, out_mode))


@pytest.mark.parametrize("src_flags", [0, F_420], ids=["422", "420"])
@pytest.mark.parametrize("flags,w,h,out_mode", SHAPES, ids=SHAPE_IDS)
def test_e_a_taller_source_in_mid_stream(flags, w, h, out_mode, src_flags):
    """Three sources of 36 rows, then 50 rows: a source slot no longer holds a frame, the rings are re-made with the slots
    they had."""
    steps = configure(8, 0) + src_height(36) + submit(6) + mark() + src_height(50) + submit(8)
    still_batched(run_script(params_of(flags, w, h), steps, w, h, 0, out_mode, src_flags=src_flags))


@pytest.mark.parametrize("flags", [["-vhs"], ["-vhs", "-tvstd", "pal"]], ids=["vhs", "pal"])
def test_f_another_frame_size_on_the_same_memory(flags):
    """One caller buffer holds a tight 256x36 frame, then a tight 192x40 frame at the same base address, then 256x36 again,
    six iterations each -- the writer table is keyed by that address.  ONE ctx throughout (`-width` binds nothing the
    engine reads: the geometry is the call's), so one engine lives across both changes."""
    w, h = 256, 36
    steps = configure(4, 0) + submit(6) + mark() + frame_is(192, 40) + submit(6) + mark() + frame_is(w, h) + submit(6)
    marks = run_script(params_of(flags, w, h), steps, w, h, 0, OUT_BOB420)
    still_batched(marks[:2])
    still_batched(marks[1:])


@pytest.mark.parametrize("flags,w,h,out_mode", SHAPES, ids=SHAPE_IDS)
def test_g_same_src_across_a_configure(flags, w, h, out_mode):
    """SUBMIT_SAME_SRC for the second field of a source whose first field went before a ntscsim_submit422_configure(): the
    device copy of the source went with the rings, so the engine takes its own (include/ntscsim.h promises the bytes of the
    in-order loop for SAME_SRC, and forbids nothing here): exact bytes, and one upload more than there are sources."""
    steps = configure(8, 0) + submit(5) + mark() + configure(4, 0) + submit(5)
    marks = run_script(params_of(flags, w, h), steps, w, h, 0, out_mode)
    still_batched(marks)
    assert marks[-1][1][2] == 5 + 1, marks[-1]


def test_h_unpin_everything_between_two_chained_iterations():
    """Page-owned planes in memory declared with ntscsim_host_pin(): the delivery kernels write the rows in place;
    ntscsim_host_unpin(ctx, NULL) in mid-stream brings the engine to rest between two chained iterations and takes the
    declaration away (the planes are staged from then on).  The rings stay, and so does the chain."""
    w, h = 256, 36
    steps = configure(4, 0) + submit(7) + unpin() + mark() + submit(7)
    marks = run_script(params_of(["-vhs"], w, h), steps, w, h, 0, OUT_BOB420, paged=True, declare=True)
    still_batched(marks)
    # (the unpin launches what is pending, into the planes that are still pinned; of the iterations of one launch that
    #  write the same rows of the one frame only the last delivers them)
    direct_before, direct_after = marks[0][1][6], marks[1][1][6] - marks[0][1][6]
    assert direct_before > 0 and direct_after == 0, marks


@pytest.mark.parametrize("name,steps", [("a", scenario_a()), ("c", scenario_c()), ("d", scenario_d())])
def test_i_controls_padded_rows_do_not_chain(name, steps):
    """The same re-makes with 16 bytes behind every row: nothing chains, so a failure here is the re-make's, not the
    chain's."""
    flags, w, h, out_mode = SHAPES[0]
    still_batched(run_script(params_of(flags, w, h), steps, w, h, 16, out_mode))


def test_i_control_narrow_tight_rows_run_one_at_a_time():
    """Scenario a at 126 wide, tight: below the width that chains every iteration runs in order on the mirror."""
    w, h = 126, 36
    marks = run_script(params_of(["-vhs"], w, h), scenario_a(), w, h, 0, OUT_BOB420)
    (n0, s0), (n1, s1) = marks
    assert (s0[3], s0[4]) == (0, n0) and (s1[3], s1[4]) == (0, n1), marks
