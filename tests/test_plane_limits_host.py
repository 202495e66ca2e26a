"""The CPU half of tests/test_plane_limits_gpu.py: the table of tests/_plane_limits.py really crosses the thresholds it is
meant for.  The product library is loaded for ntscsim_debug_fast_plane_ok() (and the draw counts) only."""
import _libs as L
import _plane_limits as PL

W, H = PL.W, PL.H


def test_n_fit_is_the_predicates_last_accepted_count():
    assert PL.n_fit(0) == 6135                   # the hand calculation: 720 * Rpad * 4 < 0xFFF00000, Lslot = 243
    for mode in (0, 1, 2):
        n = PL.n_fit(mode)
        assert PL.plane_ok(n, W, H, mode) and not PL.plane_ok(n + 1, W, H, mode)
        assert all(PL.plane_ok(k, W, H, mode) for k in range(n - 40, n)) and not any(PL.plane_ok(k, W, H, mode) for k in range(n + 1, n + 40))
    assert PL.n_fit(0) > PL.n_fit(1) > PL.n_fit(2) > PL.CHUNK
    # without head switching, and with a small one, the plane itself has bit 31 set in its last offsets
    assert PL.plane_bytes(PL.n_fit(0), W, H) > 1 << 31 and PL.plane_bytes(PL.n_fit(1), W, H) > 1 << 31
    assert PL.plane_bytes(PL.n_fit(0), W, H) < 1 << 32


def test_every_case_sits_where_it_says():
    for c in PL.CASES:
        p, n = c.params(), c.n
        assert PL.hs_mode(p, c.w) <= c.mode, c.id
        if c.at == "over":
            assert 1.05 * 2 ** 32 <= PL.plane_bytes(n, c.w, c.h) < 2 ** 33 and PL.plane_bytes(n - 1, c.w, c.h) < 1.05 * 2 ** 32, c.id
            assert PL.rpad(n, c.h) * c.w <= 1 << 31 and PL.rows(n, c.h) <= 1 << 30, c.id      # not refused
            # an index cut to 32 bits would alias whole columns, at least 30 of them
            assert (PL.plane_bytes(n, c.w, c.h) - 2 ** 32) // (PL.rpad(n, c.h) * 4) >= 30, c.id
        else:
            assert PL.plane_ok(n, c.w, c.h, c.mode) == (c.at == 0) and PL.plane_ok(n - c.at, c.w, c.h, c.mode), c.id
        # the launcher's own threshold for these switches (the mode of the displacement at hand) decides the ENCODER
        own = PL.plane_ok(n, c.w, c.h, PL.hs_mode(p, c.w))
        hand_tuned_encoder = c.forms[0].startswith(("k_encode_fast", "k_encode_fp"))
        assert own == hand_tuned_encoder, c.id
        assert n >= 4 * PL.CHUNK, c.id                                     # several small-launch twins
    assert len({c.id for c in PL.CASES}) == len(PL.CASES)
    for cid in PL.EXACT_FORMS_OF_FLOAT:
        assert PL.case(cid).sim_mode == 2 and PL.case(cid.replace("8-float", "3-vhs" if cid.endswith("fit") else "4-vhs")).forms == PL.EXACT_FORMS_OF_FLOAT[cid]


def test_head_switch_modes_of_the_switch_sets():
    tw = W + W // 10
    assert PL.hs_mode(PL.case("1-default-fit").params(), W) == 0
    for cid in ("3-vhs-fit", "7-xi-fit", "7-fo-fit", "8-float-fit"):
        p = PL.case(cid).params()
        sh = PL.head_switch_shifts(p, W)
        assert PL.hs_mode(p, W) == 1 and max(abs(s) for s in sh) <= W // 10, (cid, sh)
    # cases 5 and 6: displacements beyond W/10, one to the right and one to the left, at both ends of the noise range
    right = PL.head_switch_shifts(PL.case("5-wrap-right-fit").params(), W)
    left = PL.head_switch_shifts(PL.case("5-wrap-left-fit").params(), W)
    assert all(W // 10 < s <= tw // 2 for s in right) and all(-tw // 2 <= s < -(W // 10) for s in left), (right, left)
    for cid in ("5-wrap-right-fit", "5-wrap-left-fit", "6-wrap-right-fit+1", "6-wrap-left-fit+1"):
        c = PL.case(cid)
        assert PL.hs_mode(c.params(), W) == 2
        rp = PL.rpad(c.n, H)
        assert (W - 1 + tw) * rp * 4 > 1 << 31 and PL.plane_bytes(c.n, W, H) <= 1 << 32, cid
        # ... and the most negative offset, formed as 2^32 - k, lies above the plane
        assert (1 << 32) - tw * rp * 4 >= PL.plane_bytes(c.n, W, H) or c.at == 1, cid
    # the switch of cases 5 / 6 reaches rows of the picture: point 0.105 of 262.5 lines, 22 lines of blanking
    p = PL.case("5-wrap-right-fit").params()
    y = int(p.vhs_head_switching_point * 262.5) * 2 - 44
    assert 0 <= y < H // 4


def test_sampled_fields():
    for c in PL.CASES:
        n = c.n
        named, ks = PL.sampled_fields(n, c.h)
        ls, r = PL.lslot(c.h), PL.rows(n, c.h)
        assert len(ks) >= 8 and len(set(ks)) == len(ks) and all(0 <= k < n for k in ks), c.id
        assert named[:3] == [0, n - 1, n // 2] and all(k in ks for k in named), c.id
        wave_row, wg_row = r // 64 * 64 - 1, ((r + 62) // 63 - 1) * 63
        assert named[3] * ls <= wave_row < (named[3] + 1) * ls and (wave_row + 1) % 64 == 0 and r - 64 <= wave_row < r, c.id
        assert named[4] * ls <= wg_row < (named[4] + 1) * ls and wg_row % 63 == 0 and r - 63 <= wg_row < r, c.id
        assert {k & 1 for k in ks} == {0, 1}, c.id                          # fields of both parities
        assert len({k % PL.S for k in ks}) >= 4, c.id                      # ... from several sources
        assert len({k * 7 // n for k in ks}) >= 6, c.id                    # ... spread over the clip


def test_descriptors_pair_fields_in_shared_frames():
    n = 1201
    j = PL.jobs(n)
    assert j[0] == (0, 0, 1, 0) and j[1] == (1, 0, 0, 1) and j[n - 1] == ((n - 1) % PL.S, 600, 1, n - 1)
    keys = {(d, f) for _, d, f, _ in j}
    assert len(keys) == n and PL.S <= 8                                     # no two fields share (frame, parity)
    chunk = PL.jobs(PL.CHUNK, 600, dst_base=0)
    assert [(s, f, no) for s, _, f, no in chunk] == [(s, f, no) for s, _, f, no in j[600:1200]]
    assert [d for _, d, _, _ in chunk] == [k // 2 for k in range(PL.CHUNK)]
    p = L.make_params(["-vhs"])
    pos = PL.Positions(p, W, H)
    from ntscsim import shard
    assert all(pos(k) == shard.rng_pos_of_field(p, W, H, k) for k in (0, 1, 2, 601, 6135, 6444))


def test_refused_sizes():
    w, h, n = PL.ROWS_REFUSED
    assert PL.rows(n, h) == (1 << 30) + PL.lslot(h) and 16 <= w <= 16384 and 2 <= h <= 16384
    n = PL.n_elems_refused()
    assert PL.rpad(n, H) * W > 1 << 31 >= PL.rpad(n - 1, H) * W and PL.rows(n, H) <= 1 << 30
    assert n - 1 > PL.n_over()                                             # the "over" cases are accepted sizes


def test_peak_device_memory():
    for c in PL.CASES:
        assert c.peak_bytes() <= 16 * PL.GIB, (c.id, c.peak_bytes() / PL.GIB)
    assert max(c.peak_bytes() for c in PL.CASES) > 12 * PL.GIB             # (what the budget is about)
