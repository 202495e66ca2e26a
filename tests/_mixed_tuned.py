"""What tests/test_mixed_tuned_gpu.py shares: one ntscsim_mixed_fields_device call under ntscsim_set_mixed_forms(TUNED)
against the CPU oracle -- per descriptor, that set's parameters from that descriptor's rand() position, whole destination
buffers byte for byte --, and the kernel list such a call must report, DERIVED from what the single-set launcher picks
for each set.  The descriptors, the oracle walk and the family call are those of tests/test_mixed_fields_gpu.py."""
import numpy as np

import _libs as L
import ntscsim
import test_mixed_fields_gpu as G

FILL = G.FILL
desc = G.desc

GENERIC_ORDER = ["k_mixed_decode<false,false,%s>", "k_mixed_decode<true,true,%s>", "k_mixed_decode<true,false,%s>"]
# the hand-tuned single-set forms the mixed call has, in its launch order
TUNED_ENC = ["k_encode_fast<%s>", "k_encode_fast_pre<%s>"]
TUNED_DEC = ["k_decode_fast<false,%s>", "k_decode_fast<true,%s>", "k_decode_fast<true,%s,true>", "k_decode_fast_sv<%s>",
             "k_decode_fast_bk<false,%s>", "k_decode_fast_bk<true,%s>"]


def torch_mod():
    return G.torch_mod()


def generic_names(sets, rt="double", bob=False):
    """today's list for a call that names every set of `sets`"""
    cls = set()
    for p in sets:
        cls.add(0 if not p.emulating_vhs else (2 if p.vhs_svideo_out else 1))
    return (["k_mixed_setup", "k_mixed_encode<%s>" % rt] + [GENERIC_ORDER[c] % rt for c in sorted(cls)] +
            (["k_mixed_bob"] if bob else []))


_single = {}


def single_set_names(p, w, h, mode=None):
    """the kernels ntscsim_fields_device picks for the set on a throughput-form context, aligned buffers (cached)"""
    key = (bytes(p), w, h, mode)
    if key not in _single:
        torch = torch_mod()
        src = torch.from_numpy(np.stack([L.noise_frame(w, h, 99)])).cuda()
        dst = torch.zeros((2, h, w, 4), dtype=torch.uint8, device="cuda")
        sim = ntscsim.FieldSimulator(params=p)
        if mode is not None:
            sim.set_mode(mode)
        sim.fields(src, dst, [(0, 0, 1, 0), (0, 1, 0, 1)])
        _single[key] = sim.last_kernels()
        sim.sync()
        sim.close()
    return _single[key]


def derived_names(sets, w, h, rt="double", bob=False, mode=None):
    """The list a TUNED call over `sets` must report: each set's single-set encoder / decoder form, where it is one of
    the forms the mixed call has, under its k_mixed_ name; the generic mixed kernel (of the set's class) otherwise;
    the union in the call's fixed launch order."""
    enc, dec = set(), set()
    for p in sets:
        ran = single_set_names(p, w, h, mode)
        e = [k for k in ran if k in [t % rt for t in TUNED_ENC]]
        d = [k for k in ran if k in [t % rt for t in TUNED_DEC]]
        assert len(e) <= 1 and len(d) <= 1, ran
        enc.add(e[0].replace("k_", "k_mixed_", 1) if e else "k_mixed_encode<%s>" % rt)
        cls = 0 if not p.emulating_vhs else (2 if p.vhs_svideo_out else 1)
        dec.add(d[0].replace("k_", "k_mixed_", 1) if d else GENERIC_ORDER[cls] % rt)
    order = (["k_mixed_encode<%s>" % rt] + [t.replace("k_", "k_mixed_", 1) % rt for t in TUNED_ENC] +
             [g % rt for g in GENERIC_ORDER] + [t.replace("k_", "k_mixed_", 1) % rt for t in TUNED_DEC])
    assert enc | dec <= set(order)
    return ["k_mixed_setup"] + [k for k in order if k in enc or k in dec] + (["k_mixed_bob"] if bob else [])


def tuned_vs_oracle(sets, descs, w, h, n_src, n_dst, ctx_flags=(), start=0, pad=0, seed=0, warmup=None, prepare=None):
    """One TUNED mixed call against the oracle.  pad: extra pixels per row of both buffers (unaligned linesizes; the
    padding is compared too).  prepare(sim): further switches before the call.  Returns (last_kernels, sim-free facts)."""
    torch = torch_mod()
    ctx_params = L.make_params(list(ctx_flags))
    srcs = [L.noise_frame(w, h, 0x2345678 + seed + j) for j in range(n_src)]
    exp = np.full((n_dst, h, w, 4), FILL, np.uint8)
    end = G.Oracle().run(G.params_lookup(sets, ctx_params), descs, srcs, exp, w, h, start)
    src_pad = np.full((n_src, h, w + pad, 4), 0xC3, np.uint8)
    src_pad[:, :, :w] = np.stack(srcs)
    src_t = torch.from_numpy(src_pad).cuda()
    dst_t = torch.full((n_dst, h, w + pad, 4), FILL, dtype=torch.uint8, device="cuda")
    sim = ntscsim.FieldSimulator(params=ctx_params)
    sim.rng_pos = start
    sim.set_mixed_forms(True)
    if warmup:
        sim.debug_set_warmup(*warmup)
    if prepare:
        prepare(sim)
    arr = G.build(sim, descs, src_t[:, :, :w], dst_t[:, :, :w])
    sim.run_mixed_descs(list(sets), arr, w, h)
    names, pos, lds = sim.last_kernels(), sim.rng_pos, sim.last_decoder_lds()
    sim.sync()
    got = dst_t.cpu().numpy()
    sim.close()
    assert pos == end
    bad = [k for k in range(n_dst) if not np.array_equal(got[k, :, :w], exp[k])]
    assert not bad, "destination frames %r differ from the oracle" % bad[:10]
    if pad:
        assert (got[:, :, w:] == FILL).all(), "row padding was written"
    return names, lds
