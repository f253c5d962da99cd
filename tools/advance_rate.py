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
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "dwarf-p-cloudsc_amd"))
import cloudsc_amd as ca  # noqa: E402


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
    prec = {"fp64": ca.FP64, "mixed": ca.MIXED, "fp32": ca.FP32}[o.precision]
    outputs = {"all": ca.OUTPUTS_ALL, "surface": ca.OUTPUTS_SURFACE}[o.outputs]
    lib, hip = ca.gpu_lib(), ca._hip()
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    if o.what != "b" and not hasattr(lib, "cloudsc_gpu_run_advance"):
        sys.exit("this library has no advancing step (only --what b runs on it)")
    ds = ca.load_dataset()
    p = ca.Params.from_dict(ds.params)
    ca.check(lib.cloudsc_gpu_init(0, C.byref(p)))
    d = ca.DeviceFields(o.ngptot, o.nproma, ds.klev, prec, outputs=outputs)
    ws = C.c_void_p()
    try:
        wsb = lib.cloudsc_gpu_scratch_bytes(prec, ca.VARIANT_KSEG, o.ngptot, o.nproma, ds.klev)
        assert hip.hipMalloc(C.byref(ws), C.c_size_t(wsb)) == 0 and hip.hipMemset(ws, 0, C.c_size_t(256)) == 0
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
        for _ in range(o.warmup):
            step()
        ca.check(lib.cloudsc_gpu_check(0, None, ca.VARIANT_KSEG, ws))
        ms = []
        for _ in range(o.rounds):
            d.expand(ds)
            hip.hipDeviceSynchronize()
            t0 = time.perf_counter()
            for _ in range(o.steps):
                step()
            hip.hipDeviceSynchronize()
            ms.append(1e3 * (time.perf_counter() - t0) / o.steps)
        ca.check(lib.cloudsc_gpu_check(0, None, ca.VARIANT_KSEG, ws))
        finite = all(bool(np.isfinite(d.download_raw(k)[:o.ngptot // o.nproma]).all()) for k in ("pt", "pq", "pa", "pclv"))
        print(json.dumps({"what": o.what, "precision": o.precision, "outputs": o.outputs, "ngptot": o.ngptot,
                          "nproma": o.nproma, "steps": o.steps, "rounds": o.rounds, "finite": finite,
                          "lib": "CLOUDSC_AMD_LIB" if os.environ.get("CLOUDSC_AMD_LIB") else "this build",
                          "ms_per_step": [round(x, 4) for x in ms], "median_ms": round(statistics.median(ms), 4)}))
    finally:
        if ws.value:
            hip.hipFree(ws)
        d.close()


if __name__ == "__main__":
    main()
