"""The batched step without a GPU: the four entry points in the header, the library and the bindings; every
argument rule of cloudsc_batch_create and cloudsc_gpu_run_batch, which are all checked before the first HIP call and
so are CLOUDSC_EINVAL here too, from fake non-NULL members that are never dereferenced; the batch launch geometry;
the case table's coverage; the CLI's usage errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_cases as bc
import cloudsc_amd as ca
from host_harness import full_fields

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cloudsc_batch_create", "cloudsc_gpu_run_batch", "cloudsc_batch_nsets", "cloudsc_batch_destroy")
NOT_AEROSOL = ("plcrit_aer", "picrit_aer", "pre_ice", "pccn", "pnice")


@pytest.fixture(scope="module")
def lib():
    return ca.gpu_lib()


def test_header_library_and_bindings(lib):
    header = open(os.path.join(REPO, "include", "cloudsc_amd.h")).read()
    for name in ENTRIES + ("cloudsc_batch_launch_geometry",):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        fn = getattr(lib, name)                       # exported
        assert fn.argtypes is not None, name          # bound
    assert "typedef struct cloudsc_batch cloudsc_batch_t;" in header
    m = re.search(r"#define CLOUDSC_BATCH_MAX_SETS (\d+)", header)
    assert m and int(m.group(1)) == ca.BATCH_MAX_SETS >= 256
    assert callable(ca.Batch) and callable(ca.Batch.run) and callable(ca.Batch.close)


def sets_of(n, without=NOT_AEROSOL, step=0x100000):
    """n sets of fake members, no pointer twice (set i's are full_fields()' plus i * step)."""
    arr = (ca.Fields * n)()
    base = full_fields(without=without)
    row = np.array([getattr(base, name) or 0 for name, _ in ca.Fields._fields_], dtype=np.uint64)
    view = np.frombuffer(arr, dtype=np.uint64).reshape(n, len(row))
    view[...] = np.where(row != 0, row + np.arange(n, dtype=np.uint64)[:, None] * np.uint64(step), 0)
    return arr


def params_of(ds, n, **kw):
    arr = (ca.Params * n)()
    for i in range(n):
        arr[i] = ca.Params.from_dict(ds.params)
        for k, v in kw.items():
            setattr(arr[i], k, v)
    return arr


def create(lib, sets="default", params=None, nsets=3, precision=ca.FP64, outputs=ca.OUTPUTS_ALL, ngptot=100, nproma=16,
           klev=137, batch="own"):
    h = C.c_void_p(0x10)
    if isinstance(sets, str):
        sets = sets_of(max(nsets, 1) if nsets <= 300 else 1)
    rc = lib.cloudsc_batch_create(C.byref(h) if batch == "own" else batch, 0, precision, outputs, nsets, ngptot, nproma,
                                  klev, sets, params)
    assert h.value == 0x10 or rc == 0                 # a refused call leaves *batch alone
    return rc


@pytest.mark.parametrize("with_params", [False, True], ids=["device_set", "own_sets"])
def test_create_rules(lib, ds, with_params):
    before = lib.cloudsc_last_hip_error()

    def run(**kw):
        n = kw.get("nsets", 3)
        if with_params and "params" not in kw:
            kw["params"] = params_of(ds, n if 1 <= n <= 300 else 1)
        return create(lib, **kw)
    assert run(batch=None) == ca.EINVAL
    assert run(sets=None) == ca.EINVAL
    for nsets in (0, -1, ca.BATCH_MAX_SETS + 1, 1 << 30):
        assert run(nsets=nsets) == ca.EINVAL
    for kw in (dict(ngptot=0), dict(ngptot=-5), dict(nproma=0), dict(nproma=257), dict(nproma=(1 << 24) + 1),
               dict(klev=0), dict(klev=1), dict(precision=99), dict(precision=0), dict(outputs=2), dict(outputs=4),
               dict(outputs=-1), dict(outputs=99)):
        assert run(**kw) == ca.EINVAL, kw
    # a required member NULL in any set: every member a selection needs, in the last set
    for outputs in bc.OUTPUTS.values():
        needed = [n for n, _ in ca.Fields._fields_ if n not in NOT_AEROSOL and
                  (n not in ca.OUTPUT_FIELDS or n in ca.selected_outputs(outputs))]
        assert len(needed) == (43 if outputs == ca.OUTPUTS_ALL else 33)
        for name in needed:
            s = sets_of(3)
            setattr(s[2], name, None)
            assert run(sets=s, outputs=outputs) == ca.EINVAL, (outputs, name)
    # an aerosol input in some sets and not in others
    for name in ("picrit_aer", "pre_ice", "pnice"):
        s = sets_of(3)
        setattr(s[1], name, 0x7000)
        assert run(sets=s) == ca.EINVAL, name
    # the aliasing rule: a written member equals a member of another set, or another member of its own
    for mine, theirs, other_set in (("pcovptot", "pt", 0), ("pcovptot", "pcovptot", 0), ("plude", "plude", 0),
                                    ("plude", "pq", 1), ("tendency_loc_t", "tendency_loc_q", 2), ("pfplsl", "pap", 2),
                                    ("prainfrac_toprfz", "pfsqlf", 0), ("pfsqitur", "tendency_tmp_cld", 1)):
        s = sets_of(3)
        setattr(s[2], mine, getattr(s[other_set], theirs))
        assert run(sets=s) == ca.EINVAL, (mine, theirs, other_set)
    assert lib.cloudsc_last_hip_error() == before


def test_parameter_set_rules(lib, ds):
    assert create(lib, params=params_of(ds, 3, ncldtop=1)) == ca.EINVAL
    assert create(lib, params=params_of(ds, 3, nssopt=7)) == ca.EINVAL
    assert create(lib, params=params_of(ds, 3, ptsphy=0.0)) == ca.EINVAL
    p = params_of(ds, 3)
    p[1].laericeauto = 1                                          # one kernel per batch: aerosols in all sets or none
    assert create(lib, params=p) == ca.EINVAL
    assert create(lib, sets=sets_of(3, without=()), params=p) == ca.EINVAL
    assert create(lib, params=params_of(ds, 3, laericesed=1)) == ca.EINVAL   # aerosol kernels, no aerosol inputs


def test_what_is_allowed_passes_every_rule(lib, ds):
    """Shared inputs, NULL unselected members, aerosol inputs in every set, the most sets: never CLOUDSC_EINVAL --
    the call then succeeds, or without a device answers CLOUDSC_ENODEV."""
    ok = (0, -2)

    def run(**kw):
        h = C.c_void_p()
        n = kw.pop("nsets", 3)
        rc = lib.cloudsc_batch_create(C.byref(h), 0, kw.pop("precision", ca.FP64), kw.pop("outputs", ca.OUTPUTS_ALL), n,
                                      100, 16, 137, kw.pop("sets"), kw.pop("params", None))
        if rc == 0:
            assert lib.cloudsc_batch_nsets(h) == n
            assert lib.cloudsc_batch_destroy(h) == 0
        return rc
    p3 = params_of(ds, 3)
    s = sets_of(3)
    for name, _ in ca.Fields._fields_:                            # "one state, N parameter sets"
        if name not in ca.OUTPUT_FIELDS and name != "plude" and name not in NOT_AEROSOL:
            s[1].__setattr__(name, getattr(s[0], name))
            s[2].__setattr__(name, getattr(s[0], name))
    assert run(sets=s, params=p3) in ok
    s = sets_of(3)
    for i in range(3):
        for name in ca.DIAGNOSTIC_FLUX_FIELDS:
            setattr(s[i], name, None)
    assert run(sets=s, params=p3, outputs=ca.OUTPUTS_PROGNOSTIC) in ok
    assert run(sets=s, params=p3, outputs=ca.OUTPUTS_SURFACE, precision=ca.MIXED) in ok
    assert run(sets=sets_of(3, without=()), params=params_of(ds, 3, laericesed=1), precision=ca.FP32) in ok
    assert run(sets=sets_of(1), params=params_of(ds, 1), nsets=1) in ok
    n = ca.BATCH_MAX_SETS
    assert run(sets=sets_of(n, step=0x10000), params=None, nsets=n) in (ok + (-4,))   # (ENOINIT with a device)


def test_run_batch_judges_the_variant_before_the_batch(lib):
    fake = C.c_void_p(0x10)
    for v in (ca.VARIANT_KSEG, ca.VARIANT_SCC, ca.VARIANT_SCC_PRIVATE, 0, 77, -1, ca.VARIANT_KCACHE | 0x1000,
              ca.VARIANT_KCACHE | ca.FP32_EXACT_LIBM, ca.VARIANT_KSEG | ca.FP32_EXACT_LIBM):
        assert lib.cloudsc_gpu_run_batch(fake, None, v) == ca.EINVAL, v
    assert lib.cloudsc_gpu_run_batch(None, None, ca.VARIANT_KCACHE) == ca.EINVAL
    assert lib.cloudsc_batch_nsets(None) == ca.EINVAL
    assert lib.cloudsc_batch_destroy(None) == 0


def test_batch_launch_geometry():
    for ngptot, nproma, mode, pack in bc.SHAPES:
        ca.narrow_pack(mode)
        try:
            one = ca.launch_geometry(ca.FP64, ca.VARIANT_KCACHE, ngptot, nproma, 137)
            assert one["pack"] == pack
            for n in bc.NSETS:
                g = ca.batch_launch_geometry(ca.FP64, n, ngptot, nproma, 137)
                assert g == dict(one, units=n * one["units"], workgroups=n * one["workgroups"])
        finally:
            ca.narrow_pack(-1)
    # (40, 16) packed: ONE wave per member whose fourth sub-slot has no block -- the case the mapping must survive
    ca.narrow_pack(-1)
    assert ca.batch_launch_geometry(ca.FP64, 3, 40, 16, 137) == dict(pack=4, lanes=64, units=3, workgroups=3,
                                                                   wg_threads=64)
    for bad in (dict(nsets=0), dict(nsets=ca.BATCH_MAX_SETS + 1), dict(nproma=257), dict(precision=3)):
        kw = dict(precision=ca.FP64, nsets=3, ngptot=100, nproma=16, klev=137)
        kw.update(bad)
        with pytest.raises(ca.CloudscError):
            ca.batch_launch_geometry(**kw)


def test_the_case_table_covers_what_it_names():
    seen = lambda i: {c[i] for c in bc.CASES}
    assert seen(0) == set(bc.STATES) | {bc.AEROSOL_STATE} and seen(1) == set(bc.NSETS)
    assert {c[2:6] for c in bc.CASES} == set(bc.SHAPES)
    assert seen(6) == set(bc.PRECISIONS) and seen(7) == set(bc.OUTPUTS)
    for shape in bc.SHAPES:                              # every shape with every nsets, precision and selection
        mine = [c for c in bc.CASES if c[2:6] == shape]
        assert {c[1] for c in mine} == set(bc.NSETS)
        assert {(c[6], c[7]) for c in mine if c[0] != bc.AEROSOL_STATE} == {(p, o) for p in bc.PRECISIONS for o in bc.OUTPUTS}
    assert len(set(bc.CASES)) == len(bc.CASES)
    ps = bc.perturbed_params({"ramid": 0.8, "rcldiff": 3e-6, "x": 1})
    assert len({(p["ramid"], p["rcldiff"]) for p in ps}) == 3 and all(0 < p["ramid"] < 1 for p in ps)


CLI = os.path.join(os.path.dirname(os.path.abspath(ca.__file__)), "dwarf-cloudsc-amd")


def test_cli_batch_usage_errors():
    def run(*args):
        return subprocess.run([CLI, "1", "300", "32"] + list(args), capture_output=True, text=True, timeout=120)
    for bad in (["--batch", "3"], ["--batch", "3", "--variant", "kcache"],          # without --fields caller
                ["--batch", "3", "--fields", "caller"],                             # the default variant is kseg
                ["--batch", "3", "--fields", "caller", "--variant", "kseg"],
                ["--batch", "3", "--fields", "caller", "--variant", "scc"],
                ["--batch", "3", "--fields", "tendbuf", "--variant", "kcache"],
                ["--batch", "3", "--fields", "levels", "--variant", "kcache"],
                ["--batch", "3", "--fields", "state", "--variant", "kcache"]):
        r = run(*bad)
        assert r.returncode != 0 and "--batch goes with --fields caller and --variant kcache" in r.stderr, bad
    for bad in (["--batch", "0"], ["--batch", "x"], ["--batch", "65536"], ["--batch"]):
        r = run("--fields", "caller", "--variant", "kcache", *bad)
        assert r.returncode != 0 and "usage:" in r.stderr, bad
    assert "--batch N" in run("--help").stderr
