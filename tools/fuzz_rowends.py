"""Developer tool (GPU box): random -vhs switch sets (the draws of tools/fuzz_pipe.py) and geometries through the BATCHED launch (sim.fields: the
hand-tuned k_encode_fast / k_decode_fast pair, where the grouped row ends live) against the oracle, byte for byte,
with the method of tests/test_rowend_groups.py (_run_case).   python tools/fuzz_rowends.py 0 400"""
import collections, os, random, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "composite-video-simulator_amd"))
import numpy as np
import _libs as L
import ntscsim
import test_rowend_groups as T

s0, n = int(sys.argv[1]), int(sys.argv[2])
bad, census, t0 = [], collections.Counter(), time.time()
for seed in range(s0, s0 + n):
    r = random.Random(880000 + seed)
    flags = ["-vhs"]
    if r.random() < 0.6: flags += ["-vhs-speed", r.choice(["sp", "lp", "ep"])]
    if r.random() < 0.4: flags += ["-noise", str(r.choice([0, 1, 2, 7, 40, 100]))]
    if r.random() < 0.4: flags += ["-chroma-noise", str(r.choice([1, 3, 70, 200]))]
    if r.random() < 0.3: flags += ["-chroma-phase-noise", str(r.choice([1, 2, 9, 30]))]
    if r.random() < 0.4: flags += ["-vhs-head-switching-point", "%.4f" % r.uniform(0.6, 1.0)]
    if r.random() < 0.3: flags += ["-vhs-head-switching-phase", "%.4f" % r.uniform(0.0, 0.2)]
    if r.random() < 0.2: flags += ["-vhs-head-switching", "0"]
    if r.random() < 0.3: flags += ["-chroma-dropout", str(r.choice([100, 3000, 30000, 90000]))]
    if r.random() < 0.25: flags += ["-vhs-chroma-vblend", "0"]
    if r.random() < 0.15: flags += ["-tvstd", "pal"]
    if r.random() < 0.35: flags += [r.choice(["-comp-catv", "-comp-catv2", "-comp-catv3", "-comp-catv4"])]
    w = r.choice([33, 64, 100, 180, 256, 333, 360, 640, 719, 720, 721, 800]) if r.random() < 0.5 else r.randrange(24, 801)
    h = r.choice([2, 3, 9, 63, 64, 65, 127]) if r.random() < 0.7 else r.randrange(2, 131)
    try:
        p = L.make_params(flags, output_height=h)
        sim = ntscsim.FieldSimulator(params=p)
    except Exception:
        census["rejected switches"] += 1
        continue
    try:
        got, exp, ran = T._run_case(sim, p, w, h, seed * 7 + 1)
        census[",".join(T._chain(ran))] += 1
        if not np.array_equal(got, exp):
            bad.append((seed, flags, w, h))
    except AssertionError as e:
        bad.append((seed, flags, w, h, repr(e)[:200]))
    finally:
        sim.close()
print("fuzz_rowends: %d cases from seed %d, %d failures, %.0f s" % (n, s0, len(bad), time.time() - t0))
for k, v in census.most_common(): print("  %5d  %s" % (v, k))
for b in bad[:20]: print("  FAIL", b)
sys.exit(1 if bad else 0)
