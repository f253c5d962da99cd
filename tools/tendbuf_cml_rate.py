#!/usr/bin/env python3
"""Rate of the cumulative tendency form on one MI355X: one JSON line per run.

    tendbuf_cml_rate.py --what a|b|c [--precision fp64|mixed|fp32] [--ngptot N] [--nproma P]
                        [--steps K] [--warmup W] [--rounds R]

  a  cloudsc_gpu_run_tendbuf_outputs(PROGNOSTIC), KSEG: the step without the accumulation.  Run with
     CLOUDSC_AMD_LIB pointing at the parent commit's library it is the baseline of every claim.
  b  cloudsc_gpu_run_tendbuf_cml(PROGNOSTIC): the fused form.
  c  (a) followed by cloudsc_fields_accumulate_tendbuf on the same stream: the unfused path.

Each round times `steps` back-to-back launches between two device synchronisations on the host clock;
the line holds every round's ms per step and their median.  One process measures one thing; a caller
alternates processes and swaps their order round by round (profiles/tendbuf_cml/rate.jsonl).  The field
values drift over the steps (plude is INOUT, BUFFER_CML grows): the bytes moved do not.

EXPECTATION, written before the first run.  Byte model per column: a prognostic
step moves about 53 * KLEV elements; the fused form adds 7 * KLEV loads and stores 7 planes for 8, so
(b)/(a) should be near 1 + 6/53 = 1.11 ... 1.14 if the step were purely bandwidth-bound, and less where
it is latency- or issue-bound (fp32).  The separate pass moves 21 * KLEV elements (7 read twice, 7
written) and is a second launch, so (c)/(a) should be near 1.40 and (b)/(c) near 0.8.  Nothing here is a
pass/fail bound."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "dwarf-p-cloudsc_amd"))
import cloudsc_amd as ca  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices="abc", required=True)
    ap.add_argument("--precision", default="fp64", choices=["fp64", "mixed", "fp32"])
    ap.add_argument("--ngptot", type=int, default=163840)
    ap.add_argument("--nproma", type=int, default=128)
    ap.add_argument("--planes", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    o = ap.parse_args()
    prec = {"fp64": ca.FP64, "mixed": ca.MIXED, "fp32": ca.FP32}[o.precision]
    lib, hip = ca.gpu_lib(), ca._hip()
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    if o.what != "a" and not hasattr(lib, "cloudsc_gpu_run_tendbuf_cml"):
        sys.exit("this library has no cumulative tendency form (only --what a runs on it)")
    ds = ca.load_dataset()
    p = ca.Params.from_dict(ds.params)
    ca.check(lib.cloudsc_gpu_init(0, C.byref(p)))
    d = ca.DeviceFields(o.ngptot, o.nproma, ds.klev, prec, tend_planes=o.planes, outputs=ca.OUTPUTS_PROGNOSTIC)
    cml_buf = C.c_void_p()
    try:
        keep = []
        tmpl = ca.make_template(ds, keep)
        inputs = ca.fields_subset(d.f, [k for k in ca.INPUT_FIELDS if getattr(d.f, k, None)])
        ca.expand_fields_tendbuf(inputs, tmpl, prec, o.ngptot, o.nproma, o.planes)
        nbytes = d.tendbuf_nbytes()
        assert hip.hipMalloc(C.byref(cml_buf), C.c_size_t(nbytes)) == 0
        assert hip.hipMemset(cml_buf, 0, C.c_size_t(nbytes)) == 0
        wsb = lib.cloudsc_gpu_scratch_bytes(prec, ca.VARIANT_KSEG, o.ngptot, o.nproma, ds.klev)
        ws = C.c_void_p()
        assert hip.hipMalloc(C.byref(ws), C.c_size_t(wsb)) == 0 and hip.hipMemset(ws, 0, C.c_size_t(256)) == 0
        args = (prec, ca.VARIANT_KSEG, ca.OUTPUTS_PROGNOSTIC, o.ngptot, o.nproma, ds.klev, o.planes)
        if o.what == "a":
            def step():
                ca.gpu_run_tendbuf_outputs(d.f, *args, scratch=ws)
        else:
            cml = ca.bind_tendbuf_cml(prec, o.nproma, ds.klev, cml_buf.value)
            loc = ca.fields_subset(d.f, ["tendency_loc_t", "tendency_loc_q", "tendency_loc_a", "tendency_loc_cld"])
            if o.what == "b":
                def step():
                    ca.gpu_run_tendbuf_cml(d.f, cml, *args, scratch=ws)
            else:
                def step():
                    ca.gpu_run_tendbuf_outputs(d.f, *args, scratch=ws)
                    ca.accumulate_tendbuf(loc, cml, prec, o.ngptot, o.nproma, ds.klev, o.planes, o.planes)
        for _ in range(o.warmup):
            step()
        ca.check(lib.cloudsc_gpu_check(0, None, ca.VARIANT_KSEG, ws))
        ms = []
        for _ in range(o.rounds):
            hip.hipDeviceSynchronize()
            t0 = time.perf_counter()
            for _ in range(o.steps):
                step()
            hip.hipDeviceSynchronize()
            ms.append(1e3 * (time.perf_counter() - t0) / o.steps)
        ca.check(lib.cloudsc_gpu_check(0, None, ca.VARIANT_KSEG, ws))
        print(json.dumps({"what": o.what, "precision": o.precision, "ngptot": o.ngptot, "nproma": o.nproma,
                          "planes": o.planes, "steps": o.steps, "rounds": o.rounds,
                          "lib": "CLOUDSC_AMD_LIB" if os.environ.get("CLOUDSC_AMD_LIB") else "this build",
                          "ms_per_step": [round(x, 4) for x in ms], "median_ms": round(statistics.median(ms), 4)}))
        hip.hipFree(ws)
    finally:
        if cml_buf.value:
            hip.hipFree(cml_buf)
        d.close()


if __name__ == "__main__":
    main()
