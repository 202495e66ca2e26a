"""The exact BGRA field path (ntscsim_fields_device) at the sizes where 32-bit arithmetic stops being safe: composite
planes with bit 31 set in their buffer offsets (up to the last plane fast_plane_ok() admits, for each of its three
thresholds), the generic kernels right behind each threshold and past 2^32 bytes, launches of more than 65535 fields,
and the size and count refusals of prepare_records().  The table is tests/_plane_limits.py; tests/test_plane_limits_host.py
shows that it crosses what it claims.

Every big case asserts: the kernel forms by name; at least 8 sampled fields byte-identical to the oracle at their
closed-form rand() positions; EVERY field equal to its twin from launches of at most 600 fields (explicit positions);
memory no field owns untouched; the sources unchanged; the ctx's rand() position behind the launch."""
import numpy as np
import pytest

import _libs as L
import _plane_limits as PL
import ntscsim
from ntscsim import _capi

pytestmark = pytest.mark.gpu


def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


_oracle_fields = {}
_snapshots = {}         # rand() position -> the oracle's generator there (the stream itself does not depend on the switches)


def stream_at(p, at):
    """An oracle stream at position `at`.  The oracle reaches a position by drawing -- 10^9 draws and more for the last
    fields of a big launch, seconds of work -- so it starts from the nearest position reached before."""
    o = L.OracleStream(p)
    near = max((q for q in _snapshots if q <= at), default=None)
    if near is not None:
        o.g = L.OracleRng.from_buffer_copy(bytes(_snapshots[near]))
    o.skip(at - o.rng_pos)
    assert o.rng_pos == at
    _snapshots[at] = L.OracleRng.from_buffer_copy(bytes(o.g))
    return o


def oracle_fields(case, p, pos, ks):
    """Fields ks of the case's clip by the oracle, each at its closed-form stream position (rows of the other field:
    0); kept for the cases that share switches and fields."""
    frames = PL.sources(case.w, case.h)
    for k in sorted(ks):
        if (case.key(), k) not in _oracle_fields:
            o = stream_at(p, pos(k))
            e = np.zeros((case.h, case.w, 4), np.uint8)
            o.field(e, np.ascontiguousarray(frames[k % PL.S]), (k & 1) ^ 1, k)
            assert o.rng_pos == pos(k + 1)
            _oracle_fields[(case.key(), k)] = e
    return [_oracle_fields[(case.key(), k)] for k in ks]


def first_difference(a, b, first_field):
    """(field, row, column) of the first byte at which two clips of paired fields differ."""
    torch = torch_mod()
    ne = (a != b)
    fr = int(torch.nonzero(ne.flatten(1).any(1))[0])
    y = int(torch.nonzero(ne[fr].flatten(1).any(1))[0])
    x = int(torch.nonzero(ne[fr, y].any(1))[0])
    return first_field + 2 * fr + (0 if y & 1 else 1), y, x


class BigLaunch:
    """One launch of n fields into paired destination frames pre-filled with FILL (one guard frame behind them), from
    rand() position 0 with NTSCSIM_RNG_AUTO."""

    def __init__(self, case, n, sim_mode=None, debug=None):
        torch = torch_mod()
        self.case, self.n, self.p = case, n, case.params()
        self.w, self.h = case.w, case.h
        self.pos = PL.Positions(self.p, self.w, self.h)
        self.src = torch.from_numpy(np.array(PL.sources(self.w, self.h))).cuda()
        self.dst = torch.full(((n + 1) // 2 + 1, self.h, self.w, 4), PL.FILL, dtype=torch.uint8, device="cuda")
        self.sim = ntscsim.FieldSimulator(params=self.p)
        self.sim.set_mode(case.sim_mode if sim_mode is None else sim_mode)
        dbg = case.debug if debug is None else debug
        if dbg:
            self.sim.debug_no_fast_decode(dbg)
        self.sim.rng_pos = 0
        self.sim.fields(self.src, self.dst, PL.jobs(n))
        self.sim.sync()
        self.forms = [k for k in self.sim.last_kernels() if not k.startswith(("k_field", "k_row"))]

    def close(self):
        torch = torch_mod()
        if self.sim is not None:
            self.sim.close()
        self.sim = self.src = self.dst = None
        torch.cuda.empty_cache()

    def check_position_and_untouched(self):
        torch = torch_mod()
        n = self.n
        assert self.sim.rng_pos == self.pos(n)
        assert bool((self.dst[-1] == PL.FILL).all()), "the guard frame behind the clip was written"
        if n & 1:       # field n - 1 (an even number: field 1, the odd rows) has no partner: the even rows keep the fill
            assert bool((self.dst[(n - 1) // 2, 0::2] == PL.FILL).all()), "rows of the last frame that no field owns were written"
        assert torch.equal(self.src.cpu(), torch.from_numpy(np.array(PL.sources(self.w, self.h)))), "a source frame was written"

    def check_oracle_samples(self):
        named, ks = PL.sampled_fields(self.n, self.h)
        assert len(ks) >= 8 and all(k in ks for k in named)
        for k, e in zip(ks, oracle_fields(self.case, self.p, self.pos, ks)):
            field = (k & 1) ^ 1
            got = self.dst[k // 2].cpu().numpy()
            assert np.array_equal(got[field::2], e[field::2]), "field %d of %d differs from the oracle" % (k, self.n)

    def check_every_field_against_small_launches(self):
        torch = torch_mod()
        n = self.n
        scratch = torch.empty((PL.CHUNK // 2, self.h, self.w, 4), dtype=torch.uint8, device="cuda")
        try:
            for first in range(0, n, PL.CHUNK):
                m = min(PL.CHUNK, n - first)
                scratch.fill_(PL.FILL)
                self.sim.fields(self.src, scratch, PL.jobs(m, first, dst_base=0),
                                rng_pos=[self.pos(k) for k in range(first, first + m)])
                self.sim.sync()
                fr = (m + 1) // 2
                a, b = self.dst[first // 2:first // 2 + fr], scratch[:fr]
                if not torch.equal(a, b):
                    raise AssertionError("the launch of %d fields differs from its small-launch twin first at (field, row, column) "
                                         "%r" % (n, first_difference(a, b, first)))
        finally:
            del scratch


def exact_case(case):
    run = BigLaunch(case, case.n)
    try:
        assert run.forms == case.forms, (case.id, case.n, run.forms)
        run.check_position_and_untouched()
        run.check_oracle_samples()
        run.check_every_field_against_small_launches()
    finally:
        run.close()


EXACT = [c for c in PL.CASES if c.sim_mode == _capi.MODE_EXACT]
FLOAT = [c for c in PL.CASES if c.sim_mode == _capi.MODE_FLOAT]


@pytest.mark.parametrize("case", EXACT, ids=[c.id for c in EXACT])
def test_plane_at_and_behind_its_threshold(case):
    exact_case(case)


@pytest.mark.parametrize("case", FLOAT, ids=[c.id for c in FLOAT])
def test_float_mode_at_and_behind_its_threshold(case):
    """NTSCSIM_MODE_FLOAT: its own pipeline up to the mode-1 threshold, the FAST32 generic forms behind it -- against the
    EXACT output of the same descriptors, which is pinned to the oracle first (its every-field twin check is cases 3
    and 4, the same launch): every channel of every field within 1 LSB (the mode's stated tolerance,
    tests/test_gpu_fast_mode.py), computed on the device."""
    torch = torch_mod()
    n = case.n
    exact = BigLaunch(case, n, sim_mode=_capi.MODE_EXACT)
    fl = None
    try:
        assert exact.forms == PL.EXACT_FORMS_OF_FLOAT[case.id], exact.forms
        exact.check_position_and_untouched()
        exact.check_oracle_samples()
        exact.sim.close()           # (its composite plane goes; the destination stays)
        exact.sim = None
        fl = BigLaunch(case, n)
        assert fl.forms == case.forms, (case.id, n, fl.forms)
        fl.check_position_and_untouched()
        worst, step = 0, 256
        for f in range(0, exact.dst.shape[0], step):
            d = (exact.dst[f:f + step].to(torch.int16) - fl.dst[f:f + step].to(torch.int16)).abs().max()
            worst = max(worst, int(d))
        assert worst <= 1, "FLOAT differs from EXACT by %d LSB" % worst
    finally:
        exact.close()
        if fl is not None:
            fl.close()


# ---- counts: more fields than a grid dimension holds, tiny frames ------------------------------------------------
TW, TH = 16, 2


def _tiny_sources():
    return np.stack([L.noise_frame(TW, TH, 900 + j) for j in range(PL.S)])


def test_65540_fields_without_bob():
    """More fields than k_bob's grid could take, none of them asking for it: every field against the oracle in one
    pass of its stream."""
    torch = torch_mod()
    n = 65540
    p = L.make_params(["-vhs"])
    frames = _tiny_sources()
    o = L.OracleStream(p)
    exp = np.zeros((n, TH, TW, 4), np.uint8)
    for k in range(n):
        o.field(exp[k], frames[k % PL.S], (k & 1) ^ 1, k)
    sim = ntscsim.FieldSimulator(params=p)
    try:
        src = torch.from_numpy(frames).cuda()
        dst = torch.zeros((n, TH, TW, 4), dtype=torch.uint8, device="cuda")
        sim.fields(src, dst, [(k % PL.S, k, (k & 1) ^ 1, k) for k in range(n)])
        sim.sync()
        got = dst.cpu().numpy()
        bad = np.nonzero((got != exp).reshape(n, -1).any(1))[0]
        assert bad.size == 0, "first wrong field: %d of %d" % (bad[0], n)
        assert sim.rng_pos == o.rng_pos
        assert "k_bob" not in sim.last_kernels()
    finally:
        sim.close()
        del sim
        torch.cuda.empty_cache()


def test_65535_fields_with_bob():
    """The largest count k_bob's grid takes (one grid row per field): every frame against the oracle's field + bob."""
    torch = torch_mod()
    n = 65535
    p = L.make_params(["-vhs"])
    frames = _tiny_sources()
    o = L.OracleStream(p)
    exp = np.full((n, TH, TW, 4), 0x33, np.uint8)
    bob = L.oracle().ntsc_oracle_bob
    for k in range(n):
        o.field(exp[k], frames[k % PL.S], (k & 1) ^ 1, k)
        bob(L._ptr(exp[k]), TW * 4, TW, TH, (k & 1) ^ 1)
    sim = ntscsim.FieldSimulator(params=p)
    try:
        src = torch.from_numpy(frames).cuda()
        dst = torch.full((n, TH, TW, 4), 0x33, dtype=torch.uint8, device="cuda")
        sim.fields(src, dst, [(k % PL.S, k, (k & 1) ^ 1, k) for k in range(n)], bob=True)
        sim.sync()
        assert "k_bob" in sim.last_kernels()
        got = dst.cpu().numpy()
        bad = np.nonzero((got != exp).reshape(n, -1).any(1))[0]
        assert bad.size == 0, "first wrong frame: %d of %d" % (bad[0], n)
        assert sim.rng_pos == o.rng_pos
    finally:
        sim.close()
        del sim
        torch.cuda.empty_cache()


def _refused(sim, descs, n, w, h, watched):
    """The call is refused with NTSCSIM_E_SIZE; the rand() position and the watched tensors are as they were."""
    torch = torch_mod()
    before = [t.clone() for t in watched]
    sim.rng_pos = 12345
    rc = L.product().ntscsim_fields_device(sim._h, descs, n, w, h, None)
    assert rc == _capi.E_SIZE, rc
    sim.sync()
    assert sim.rng_pos == 12345
    for t, b in zip(watched, before):
        assert torch.equal(t, b)


def _small_launch_equals_oracle(sim, p):
    """The next valid launch on the same ctx (4 fields of 96 x 32 from position 0)."""
    torch = torch_mod()
    w, h, n = 96, 32, 4
    frames = np.stack([L.noise_frame(w, h, 40 + j) for j in range(2)])
    o = L.OracleStream(p)
    exp = np.zeros((n, h, w, 4), np.uint8)
    for k in range(n):
        o.field(exp[k], frames[k // 2], (k & 1) ^ 1, k)
    src = torch.from_numpy(frames).cuda()
    dst = torch.zeros((n, h, w, 4), dtype=torch.uint8, device="cuda")
    sim.rng_pos = 0
    sim.fields(src, dst, [(k // 2, k, (k & 1) ^ 1, k) for k in range(n)])
    sim.sync()
    assert np.array_equal(dst.cpu().numpy(), exp) and sim.rng_pos == o.rng_pos


def test_65536_fields_with_one_bob_descriptor_are_refused():
    torch = torch_mod()
    n = 65536
    p = L.make_params(["-vhs"])
    sim = ntscsim.FieldSimulator(params=p)
    try:
        src = torch.from_numpy(_tiny_sources()).cuda()
        dst = torch.full((n, TH, TW, 4), PL.FILL, dtype=torch.uint8, device="cuda")
        d = sim.build_descs(src, dst, [(k % PL.S, k, (k & 1) ^ 1, k) for k in range(n)])
        d[40000].flags |= _capi.DESC_BOB
        _refused(sim, d, n, TW, TH, [src, dst])
        _small_launch_equals_oracle(sim, p)
    finally:
        sim.close()
        del sim
        torch.cuda.empty_cache()


@pytest.mark.parametrize("what", ["rows", "elements"])
def test_sizes_beyond_the_plane_limits_are_refused(what):
    """R = 2^30 + Lslot rows, and the smallest count with Rpad * W > 2^31 elements: NTSCSIM_E_SIZE, decided before a
    descriptor is read, so every descriptor names one real frame pair.  Nothing is launched."""
    torch = torch_mod()
    w, h, n = PL.ROWS_REFUSED if what == "rows" else (PL.W, PL.H, PL.n_elems_refused())
    p = L.make_params(["-vhs"])
    sim = ntscsim.FieldSimulator(params=p)
    try:
        src = torch.from_numpy(np.ascontiguousarray(L.noise_frame(w, h, 7)[None])).cuda()
        dst = torch.full((1, h, w, 4), PL.FILL, dtype=torch.uint8, device="cuda")
        d = sim.build_descs(src, dst, [(0, 0, (k & 1) ^ 1, k) for k in range(n)])
        _refused(sim, d, n, w, h, [src, dst])
        _small_launch_equals_oracle(sim, p)
    finally:
        sim.close()
        del sim
        torch.cuda.empty_cache()
