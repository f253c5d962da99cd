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
import contextlib
import json
import sys

import rate_harness as rh
from rate_harness import ca


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
    prec = rh.PRECISION[o.precision]
    lib, hip = ca.gpu_lib(), rh.hip_api()
    if o.what != "a" and not hasattr(lib, "cloudsc_gpu_run_tendbuf_cml"):
        sys.exit("this library has no cumulative tendency form (only --what a runs on it)")
    ds = ca.load_dataset()
    rh.gpu_init(lib, ds)
    d = ca.DeviceFields(o.ngptot, o.nproma, ds.klev, prec, tend_planes=o.planes, outputs=ca.OUTPUTS_PROGNOSTIC)
    with contextlib.closing(d):
        keep = []
        tmpl = ca.make_template(ds, keep)
        inputs = ca.fields_subset(d.f, [k for k in ca.INPUT_FIELDS if getattr(d.f, k, None)])
        ca.expand_fields_tendbuf(inputs, tmpl, prec, o.ngptot, o.nproma, o.planes)
        with rh.device_buffer(hip, d.tendbuf_nbytes(), fill=0) as cml_buf, \
                rh.kseg_workspace(lib, hip, prec, ca.VARIANT_KSEG, o.ngptot, o.nproma, ds.klev) as ws:
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
            ms = rh.what_rounds(hip, step, o, rh.launch_check(lib, ca.VARIANT_KSEG, ws))
            keys = ("what", "precision", "ngptot", "nproma", "planes", "steps", "rounds")
            print(json.dumps(rh.what_record(o, ms, keys)))


if __name__ == "__main__":
    main()
