"""The dwarf's stdout contract, checked the way the reference's benchmark
harness reads it: JUBE's `timing_pattern` and `results_pattern`
(benchmark/include/include_patternset.yml:2-171) applied to captured
`dwarf-cloudsc-amd` output.

The patterns are restated here, not copied: the per-field result patterns are
generated from the field list (the yml spells out one block of five per field,
:10-134), and JUBE's default `$jube_pat_*` macros are expanded to their
documented regexes.  The reference C validator prints the tendency rows in
upper case (`TENDENCY_LOC%A`, src/cloudsc_c/cloudsc/cloudsc_validate.c:213-216)
while the yml spells the Fortran dwarf's `tendency_loc%a`; those four rows are
matched case-insensitively, the P* rows exactly.

CPU: the `--variant cpu` run prints one `@ core#` row per host thread like the
C dwarf (cloudsc_driver.c:238-253).  GPU (tests/test_gpu_driver.py): the
`--gpus N` shard rows end in `@ core#` like the reference GPU driver
(src/cloudsc_cuda/cloudsc/cloudsc_driver.cu:475)."""
import os
import re
import subprocess

import pytest

import cloudsc_amd as ca
from host_harness import TIMING, check_results, check_timing, jube

def test_jube_macros_expand():
    assert re.fullmatch(jube("$jube_pat_fp"), "-0.1026720108982E-03")
    assert re.fullmatch(jube("$jube_pat_nint"), "-1")
    assert "$" not in jube(TIMING["thr_time"])


def test_jube_patterns_on_cpu_dwarf():
    """`dwarf-cloudsc-amd 3 2000 32 --variant cpu`: three `@ core#` thread rows,
    one TOTAL row with NUMOMP/NGPTOT/#BLKS/NPROMA, and all 21 x 5 result values."""
    exe = os.path.join(os.path.dirname(ca.LIB_PATH), "dwarf-cloudsc-amd")
    if not os.path.exists(exe):
        pytest.skip("dwarf-cloudsc-amd not built")
    r = subprocess.run([exe, "3", "2000", "32", "--variant", "cpu", "--reps", "2"], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout[-4000:], r.stderr[-1000:])
    assert r.returncode == 0
    _, tot = check_timing(r.stdout, 3, 2000, 32, 63)
    assert tot["tot_numomp"] == [3]
    # the threads' columns add up to NGPTOT (the #GP-cols column of the thread rows)
    rows = re.findall(r"^\s+3\s+2000\s+(\d+)\s+(\d+)\s+32\s+(\d) :.*@ core#$", r.stdout, re.M)
    assert sorted(int(t) for _, _, t in rows) == [0, 1, 2]
    assert sum(int(c) for c, _, _ in rows) == 2000 and sum(int(b) for _, b, _ in rows) == 63
    check_results(r.stdout)
