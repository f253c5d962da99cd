#!/usr/bin/env python3
"""Rate of the per-column multiplier form (SPP) on one MI355X: one JSON line per run.

    spp_rate.py --what a|b [--precision fp64|mixed|fp32] [--variant kseg|kcache] [--ngptot N] [--nproma P]
                [--steps K] [--warmup W] [--rounds R]

  a  cloudsc_gpu_run_outputs(ALL): the ordinary step.  Run with CLOUDSC_AMD_LIB pointing at the parent commit's
     library it is the baseline of every claim; run on this build it shows whether the ordinary step moved.
  b  cloudsc_gpu_run_spp(ALL) with all five members set to seeded multipliers in [0.75, 1.25].

Each round times `steps` back-to-back launches between two device synchronisations on the host clock; the line
holds every round's ms per step and their median.  One process measures one thing; a caller alternates processes
and swaps their order round by round (profiles/spp/rate.jsonl).  plude is INOUT and drifts over the steps: the
bytes moved do not.

EXPECTATION, written before the first run.  (a) on this build against (a) on the parent's library: the same
kernels by the compiler's resource table, so any difference must lie inside the spread the parent shows against
itself from process to process (placement of the field set varies from process to process).  (b)/(a): the form
reads five surface fields more, 40 B per column in fp64 against about 56,036 B, so the byte model
says 1 + 40/56036 = 1.0007: nothing.  What the form can cost beyond that is in the level loop: it reads a
multiplier again at each of its four uses at every physics level (four vector loads from fields that stay in
L2, each waited for where it is used, since nothing is carried in registers) and does five multiplies per level.
With about 2.5 waves per SIMD to hide a load's latency behind, a few per cent would not surprise; more than
that would say the waits are exposed.  fp32, whose level loop is bound by VALU issue and which keeps its
parameter block in VGPRs, may pay more than fp64.  Nothing here is a pass/fail bound."""
import argparse
import contextlib
import json
import sys

import numpy as np

import rate_harness as rh
from rate_harness import ca


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices="ab", required=True)
    ap.add_argument("--precision", default="fp64", choices=["fp64", "mixed", "fp32"])
    ap.add_argument("--variant", default="kseg", choices=["kseg", "kcache"])
    ap.add_argument("--ngptot", type=int, default=163840)
    ap.add_argument("--nproma", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    o = ap.parse_args()
    prec, variant = rh.PRECISION[o.precision], rh.VARIANT[o.variant]
    lib, hip = ca.gpu_lib(), rh.hip_api()
    if o.what == "b" and not hasattr(lib, "cloudsc_gpu_run_spp"):
        sys.exit("this library has no per-column multiplier form (only --what a runs on it)")
    ds = ca.load_dataset()
    rh.gpu_init(lib, ds)
    d = ca.DeviceFields(o.ngptot, o.nproma, ds.klev, prec)
    with contextlib.closing(d), contextlib.ExitStack() as mult:
        d.expand(ds)
        ws = mult.enter_context(rh.kseg_workspace(lib, hip, prec, variant, o.ngptot, o.nproma, ds.klev))
        args = (prec, variant, ca.OUTPUTS_ALL, o.ngptot, o.nproma, ds.klev)
        if o.what == "a":
            def step():
                ca.gpu_run_outputs(d.f, *args, scratch=ws)
        else:
            rng = np.random.default_rng(o.seed)
            n = ca.nblocks_of(o.ngptot, o.nproma) * o.nproma
            fields = [rng.uniform(0.75, 1.25, n).astype(ca.storage_dtype(prec)) for _ in ca.SPP_SLOTS]
            spp = ca.Spp(*[mult.enter_context(rh.device_buffer(hip, a.nbytes, fill=a)).value for a in fields])

            def step():
                ca.gpu_run_spp(d.f, spp, *args, scratch=ws)
        ms = rh.what_rounds(hip, step, o, rh.launch_check(lib, variant, ws))
        keys = ("what", "precision", "variant", "ngptot", "nproma", "steps", "rounds")
        print(json.dumps(rh.what_record(o, ms, keys)))


if __name__ == "__main__":
    main()
