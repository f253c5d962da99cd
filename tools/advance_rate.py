#!/usr/bin/env python3
"""Rate of the advancing step on one MI355X: one JSON line per run.

    advance_rate.py --what a|b|c [--precision fp64|mixed|fp32] [--outputs all|surface] [--ngptot N] [--nproma P]
                    [--steps K] [--warmup W] [--rounds R]

  a  cloudsc_gpu_run_advance in place, KSEG: the new state stored instead of the seven local tendencies.
  b  cloudsc_gpu_run_outputs of the same selection on the same set: the ordinary step.  Run with
     CLOUDSC_AMD_LIB pointing at the parent commit's library it is the yardstick.
  c  (b) followed by cloudsc_fields_advance in place on the same stream: the unfused path.

Each round times `steps` back-to-back launches between two device synchronisations on the host clock; the
line holds every round's ms per step and their median.  One process measures one thing; a caller alternates
processes and swaps their order round by round.  In (a) and (c) the state is integrated in time, with the
template's incoming tendencies applied every step, so the set is filled again from the template before the
warm-up and before every round (outside the timed region): no round integrates more than `steps` time steps,
and the line says whether pt, pq, pa and pclv were all finite after the last round ("finite").  A round whose
state left the finite range would not be comparable with (b).

EXPECTATION, written before the first run.  The advancing step stores seven planes per level (t, q, a, four
condensates; no vapour plane) where the ordinary step stores eight (the vapour tendency's zeros included) and
reads nothing twice, so by bytes (a)/(b) is 1.00 or just below.  The pass reads 3 x 7 planes and writes 7 per
level, 28 of a step's about 56 element planes, and is a second launch: (c)/(b) should be near 1.5 and (a)/(c)
near 0.65.  Nothing here is a pass/fail bound."""
import argparse
import contextlib
import json
import sys

import numpy as np

import rate_harness as rh
from rate_harness import ca


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices="abc", required=True)
    ap.add_argument("--precision", default="fp64", choices=["fp64", "mixed", "fp32"])
    ap.add_argument("--outputs", default="all", choices=["all", "surface"])
    ap.add_argument("--ngptot", type=int, default=163840)
    ap.add_argument("--nproma", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    o = ap.parse_args()
    prec, outputs = rh.PRECISION[o.precision], rh.OUTPUTS[o.outputs]
    lib, hip = ca.gpu_lib(), rh.hip_api()
    if o.what != "b" and not hasattr(lib, "cloudsc_gpu_run_advance"):
        sys.exit("this library has no advancing step (only --what b runs on it)")
    ds = ca.load_dataset()
    rh.gpu_init(lib, ds)
    d = ca.DeviceFields(o.ngptot, o.nproma, ds.klev, prec, outputs=outputs)
    with contextlib.closing(d), rh.kseg_workspace(lib, hip, prec, ca.VARIANT_KSEG, o.ngptot, o.nproma, ds.klev) as ws:
        args = (prec, ca.VARIANT_KSEG, outputs, o.ngptot, o.nproma, ds.klev)
        if o.what == "b":
            def step():
                ca.gpu_run_outputs(d.f, *args, scratch=ws)
        else:
            adv = ca.Advance.in_place(d.f)
            if o.what == "a":
                def step():
                    ca.gpu_run_advance(d.f, adv, *args, scratch=ws)
            else:
                def step():
                    ca.gpu_run_outputs(d.f, *args, scratch=ws)
                    ca.advance_fields(d.f, adv, prec, o.ngptot, o.nproma, ds.klev)
        d.expand(ds)
        ms = rh.what_rounds(hip, step, o, rh.launch_check(lib, ca.VARIANT_KSEG, ws), before_round=lambda: d.expand(ds))
        finite = all(bool(np.isfinite(d.download_raw(k)[:o.ngptot // o.nproma]).all()) for k in ("pt", "pq", "pa", "pclv"))
        keys = ("what", "precision", "outputs", "ngptot", "nproma", "steps", "rounds", "finite")
        print(json.dumps(rh.what_record(o, ms, keys, finite=finite)))


if __name__ == "__main__":
    main()
