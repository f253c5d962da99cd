#!/usr/bin/env python3
"""Line coverage of the oracle's kernel function on sets of states (CPU only; gcc + gcov).

Compiles oracle/cloudsc_oracle.c with --coverage into a temporary directory, runs every state of a set
through it (100 columns, fp64, one thread; one child process per set, so that the counters of the sets
stay apart) and prints, per set, the share of cloudsc_oracle_block_dp's executable lines that ran and the
line ranges that did not.  The sets:

    shipped   the shipped state alone
    table     the states of tests/form_state_cases.py (the kernel forms are pinned on these)
    parity    every state the plain kernels are pinned on in tests/test_gpu_parity.py

and the check that matters: every line `parity` reaches, `table` reaches too (exit status 1 if not).

    python tools/oracle_coverage.py
"""
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("tests", "dwarf-p-cloudsc_amd", "oracle", "tools"):
    sys.path.insert(0, os.path.join(REPO, d))

KERNEL = "cloudsc_oracle_block_dp"
SETS = ("shipped", "table", "parity")


def build(tmp):
    src = os.path.join(REPO, "oracle", "cloudsc_oracle.c")
    flags = ["-O0", "--coverage", "-fPIC", "-fopenmp", "-ffp-contract=off", "-std=gnu11",
             "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "oracle")]
    for obj, extra in (("oracle_dp.o", []), ("oracle_sp.o", ["-DORACLE_SP"])):
        subprocess.check_call(["gcc"] + flags + extra + ["-c", src, "-o", os.path.join(tmp, obj)])
    lib = os.path.join(tmp, "liboracle_cov.so")
    subprocess.check_call(["gcc", "-shared", "-fopenmp", "--coverage", os.path.join(tmp, "oracle_dp.o"),
                           os.path.join(tmp, "oracle_sp.o"), "-o", lib, "-lm"])
    return lib


def states_of(which):
    """[(name, Dataset)] of a set."""
    import cloudsc_amd as ca
    import make_fixtures as mf
    ds = ca.load_dataset()
    scenarios = {n: mf.load_scenario(n, ds) for n in ("W", "M")}
    if which == "shipped":
        return [("shipped", ds)]
    if which == "table":
        import form_state_cases as fs
        return [(n, fs.dataset(n, ds, scenarios)) for n in fs.STATES]
    from test_mixed_cpu import configured
    out = [("shipped", ds), ("W", scenarios["W"]), ("M", scenarios["M"])]
    out += [("seed%d" % i, mf.perturbed(ds, i)) for i in (1, 2, 3)]
    out += [(c, configured(ds, c)) for c in ("nssopt0", "nssopt2", "nssopt3", "aerosol", "ncldtop2", "ncldtop40",
                                             "ncldtop120", "ncldtop137", "ncldtop138", "cold", "dry", "moist",
                                             "klev3", "klev16")]
    flags = ds.copy()
    flags.params.update(laericesed=1, laericeauto=1)
    divisors = ds.copy()
    for name, f in (("rtaumel", 0.7310432), ("rdepliqrefdepth", 1.913), ("rvrfactor", 1.3370001), ("rd", 1.0000137)):
        divisors.params[name] *= f
    out += [("aerosol_flags", flags), ("divisor_params", divisors), ("klev60", mf.sliced_levels(ds, 77)),
            ("klev274", mf.refined_levels(ds, 2))]
    out += [(c, mf.edge_case(ds, c)) for c in mf.EDGE_CASES]
    out += [(c, mf.param_case(ds, c)) for c in mf.PARAM_CASES]
    return out


def child(which, lib):
    import oracle
    oracle.use_oracle_library(lib)
    for name, s in states_of(which):
        oracle.run_oracle(s, 100, 64, nthreads=1)


def kernel_lines(tmp):
    """{line: executed?} of the kernel function, from gcov's JSON for the fp64 object."""
    js = subprocess.check_output(["gcov", "--json-format", "--stdout", os.path.join(tmp, "oracle_dp.gcda")], cwd=tmp)
    lines = {}
    for f in json.loads(js)["files"]:
        if os.path.basename(f["file"]) != "cloudsc_oracle.c":
            continue
        for ln in f["lines"]:
            if ln.get("function_name") == KERNEL:
                lines[ln["line_number"]] = lines.get(ln["line_number"], False) or ln["count"] > 0
    return lines


def ranges(nums):
    out, nums = [], sorted(nums)
    for n in nums:
        if out and n == out[-1][1] + 1:
            out[-1][1] = n
        else:
            out.append([n, n])
    return ", ".join("%d" % a if a == b else "%d-%d" % (a, b) for a, b in out)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3])
    covered, total = {}, None
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)
        for which in SETS:
            for f in os.listdir(tmp):
                if f.endswith(".gcda"):
                    os.remove(os.path.join(tmp, f))
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", which, lib])
            lines = kernel_lines(tmp)
            total = set(lines)
            covered[which] = {n for n, hit in lines.items() if hit}
    for which in SETS:
        c = covered[which]
        print("%-8s %5.1f %%  (%d of %d executable lines of %s)" % (which, 100.0 * len(c) / len(total), len(c),
                                                                    len(total), KERNEL))
        print("         not reached: oracle/cloudsc_oracle.c:%s" % (ranges(total - c) or "-"))
    missing = covered["parity"] - covered["table"]
    print("lines `parity` reaches and `table` does not: %s" % (ranges(missing) or "none"))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
