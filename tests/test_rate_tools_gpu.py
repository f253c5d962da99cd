"""The ten tools/*_rate.py end to end on the device, each as a fresh child process at the smallest shape that
still takes every path: exit status, one JSON record per stdout line, the order of the record kinds, and per kind
the key set of the same kind in the committed profile -- what keeps a new run comparable with profiles/ line
for line.  No time and no ratio is asserted: at 8192 columns they mean nothing.  The three field-rate tools
have no --nproma / --rounds / --warmup; their shape is --ngptot 8192 --reps 2.

The children run one after another.  One that ends on a signal, on 124 / 134 / 137 / 139 or at its limit stops
the module: every later case is skipped with that reason, nothing is tried again."""
# Per-child limit: on one MI355X the tools of the parent commit took, at these arguments, 0.30 to 1.39 s per
# process, start of the interpreter and load of the library included (the slowest: tendbuf_rate.py, 1.39 s, the first
# process of the session; the --what processes about 0.5 s, the other in-process tools 0.9 to 1.2 s).  The limit is
# twice the slowest, 2.78 s, rounded up to whole seconds.
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 3
SHAPE = ["--ngptot", "8192", "--nproma", "64", "--rounds", "2", "--warmup", "1"]
FIELD_SHAPE = ["--ngptot", "8192", "--reps", "2"]
WHAT_KEYS = {"what", "precision", "ngptot", "nproma", "steps", "rounds", "lib", "ms_per_step", "median_ms"}
# the parent's json.dumps call in spp_rate.py (profiles/spp/rate.jsonl holds wrapped lines, not tool records)
SPP_KEYS = WHAT_KEYS | {"variant"}
HEAD = ["expectation", "stream_copy"]

# id: (tool, arguments, profile under profiles/ or a literal key set, the record kinds in order)
CASES = {
    "tendbuf_rate": ("tendbuf_rate", SHAPE, "tendbuf/tendbuf_rate.jsonl", HEAD + ["kseg_tendbuf"] * 3),
    "outputs_rate": ("outputs_rate", SHAPE, "outputs/outputs_rate.jsonl", HEAD + ["kseg_outputs"] * 3),
    "outputs_surface_rate": ("outputs_surface_rate", SHAPE, "outputs_surface/outputs_surface_rate.jsonl",
                             HEAD + ["kseg_outputs_surface"] * 3),
    "tendbuf_outputs_rate": ("tendbuf_outputs_rate", SHAPE, "tendbuf_outputs/rate.jsonl",
                             HEAD + ["kseg_tendbuf_outputs", "validate_tendbuf"] * 3),
    "convert_rate": ("convert_rate", FIELD_SHAPE, "fields_convert/convert_rate.jsonl",
                     ["stream_copy"] + ["convert"] * 12 + ["reblock_round_trip"]),
    "fields_compare_rate": ("fields_compare_rate", FIELD_SHAPE, "fields_compare/compare_rate.jsonl",
                            ["stream_copy", "compare", "download_and_numpy"] + ["compare"] * 3
                            + ["fields_validate", "validate_wall"]),
    "fields_layout_rate": ("fields_layout_rate", FIELD_SHAPE, "fields_layout/rate.jsonl",
                           ["stream_copy"] + ["plain_convert"] * 2 + ["convert_layout"] * 10 + ["levels_round_trip"]),
    "fields_layout_rate-ab": ("fields_layout_rate", FIELD_SHAPE + ["--ab", "--label", "lds"],
                              "fields_layout/rate_ab.jsonl", ["layout_ab"]),
}
for _tool, _letters, _keys in (("tendbuf_cml_rate", "abc", "tendbuf_cml/rate.jsonl"), ("spp_rate", "ab", SPP_KEYS),
                               ("advance_rate", "abc", "advance/rate.jsonl")):
    for _w in _letters:
        CASES["%s-%s" % (_tool, _w)] = (_tool, SHAPE + ["--steps", "2", "--what", _w], _keys, [_w])

_stopped = []                                   # the reason, once a child has died or hung


def kind(rec):
    return rec.get("measure", rec.get("what"))


def profile_keys(path):
    """kind -> key set, from the first record of each kind in a committed profile."""
    keys = {}
    with open(os.path.join(REPO, "profiles", path)) as fh:
        for line in fh:
            rec = json.loads(line)
            keys.setdefault(kind(rec), set(rec))
    return keys


@pytest.mark.parametrize("case", list(CASES))
def test_rate_tool_emits_the_records_of_its_profile(case):
    if _stopped:
        pytest.skip(_stopped[0])
    tool, args, profile, kinds = CASES[case]
    cmd = [sys.executable, os.path.join(REPO, "tools", tool + ".py")] + args
    try:
        r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _stopped.append("%s did not end within %d s: no further process is started on the device" % (case, CHILD_TIMEOUT_S))
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _stopped.append("%s ended with status %d: no further process is started on the device" % (case, r.returncode))
    assert r.returncode == 0, r.stderr[-2000:]
    recs = [json.loads(line) for line in r.stdout.splitlines()]          # every line is one record
    assert [kind(x) for x in recs] == kinds
    want = profile_keys(profile) if isinstance(profile, str) else {k: profile for k in kinds}
    for rec in recs:
        assert set(rec) == want[kind(rec)], kind(rec)
