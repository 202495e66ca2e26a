#!/usr/bin/env python3
"""tools/float_model_err.py -- how far an fp32 evaluation of NTSCSIM_MODE_FLOAT's definition is from the definition.

For exactly the FLOAT cases of tests/test_float_model_gpu.py (tests/_modes.py: FLOAT_CASES whose form is "fp", and the
long batch) it evaluates the model's real32 and real64 flavours (oracle/ntsc_modes_oracle.c) and prints, per case and
overall, the largest |v32 - v64| of the channel values in front of the final truncation (output LSB) and the largest
difference of the composite plane (units of the 256-scaled signal).  The GPU tests' tolerances are 4 x the overall
maxima.  Runs on the CPU and needs no GPU.  Prerequisite: the whole build (`__graft_entry__.build()`), not
the oracle alone -- the switches of a case are parsed by the product library's own parser (libntscsim.so, loaded through
the ntscsim package, which imports torch where it is installed).
  python tools/float_model_err.py > profiles/float_model_err.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def main():
    import _libs as L
    import _modes as M
    cases = [c for c in M.FLOAT_CASES if c[6] == "fp"] + [M.LONG_BATCH + ("fp", {})]
    print("# real32 against real64 (oracle/ntsc_modes_oracle.c), one line per FLOAT case of tests/test_float_model_gpu.py")
    print("# %-22s %5s %5s %4s  %-14s %-14s" % ("case", "W", "H", "n", "max|dv| [LSB]", "max|dcomp| [1/256]"))
    worst_v = worst_c = 0.0
    for name, flags, w, h, n, kind, form, extra in cases:
        p = L.make_params(flags)
        srcs = M.sources(kind, w, h)
        il, tff = extra.get("interlaced", 0), extra.get("tff", 0)
        a, b = M.ModelStream(p, "real64"), M.ModelStream(p, "real32")
        dv = dc = 0.0
        for si, field, fieldno in M.jobs(n, len(srcs)):
            da, db = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 4), np.uint8)
            oa = a.field(da, srcs[si], field, fieldno, il, tff)
            ob = b.field(db, srcs[si], field, fieldno, il, tff)
            assert a.rng_pos == b.rng_pos
            if oa["v"].size:
                dv = max(dv, float(np.abs(oa["v"] - ob["v"].astype(np.float64)).max()))
                dc = max(dc, float(np.abs(oa["composite"] - ob["composite"].astype(np.float64)).max()))
        print("  %-22s %5d %5d %4d  %-14.6f %-14.6f" % (name, w, h, n, dv, dc))
        worst_v, worst_c = max(worst_v, dv), max(worst_c, dc)
    print("overall max|dv|    = %.6f LSB      -> DELTA_OUT  = 4 x = %.6f  (ceiling 1/16 = 0.0625)" % (worst_v, 4 * worst_v))
    print("overall max|dcomp| = %.6f units    -> DELTA_COMP = 4 x = %.6f  (ceiling 0.25)" % (worst_c, 4 * worst_c))
    return 0 if 4 * worst_v <= 1.0 / 16 and 4 * worst_c <= 0.25 else 1


if __name__ == "__main__":
    sys.exit(main())
