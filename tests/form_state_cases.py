"""TEST INFRASTRUCTURE ONLY -- the states on which the kernel forms (the tendency
buffer form, the prognostic-outputs form, the packed form) are pinned, named
once: the committed scenarios W and M (rain, melting, freezing, land), the
perturbed seeds, the regime copies, input and parameter edges of the shipped
state, aerosols on W, the other NSSOPT on W and M, and other NCLDTOP / KLEV on W's
inputs.  tools/oracle_coverage.py measures that these states reach every line of the
oracle's kernel that the states of tests/test_gpu_parity.py reach (NSSOPT 0 and 2 are
here for that).

Every state carries what the fp64 oracle must show on it (ACTIVITY, asserted once
per state in tests/test_forms_states_cpu.py), so that a state cannot go quiet
unnoticed.  The expectations come from the committed goldens (scenario_W.npz:
2859 non-zero pfplsl; scenario_M.npz: 100 columns of prainfrac_toprfz) and from
oracle runs, never from the kernels.  Nothing here calls the library under test."""
import numpy as np

import cloudsc_amd as ca
import make_fixtures as mf
from host_harness import configured, uses_aerosols  # noqa: F401

NGPTOT = 100                      # the template's columns, each once
ORACLE_NPROMA = 64                # the oracle's columns do not depend on the blocking
NAMES = [k for _, k in ca.VALIDATED]
QR = 2                            # rain in tendency_loc_cld[5]

GOLDEN_W_PFPLSL_NONZERO = 2859
GOLDEN_M_TOPRFZ_COLUMNS = 100


def _levels_on_w(w, case):
    if case == "klev60":
        return mf.sliced_levels(w, w.klev - 60)         # NCLDTOP as shipped
    if case == "klev3":
        return configured(w, "klev3")                    # NCLDTOP 2
    if case == "klev274":
        return mf.refined_levels(w, 2)
    return configured(w, case)                           # ncldtop<N>


# name -> (base, builder(base dataset)); base "ds" is the shipped state
BUILDERS = {
    "W": ("W", lambda s: s),
    "M": ("M", lambda s: s),
    "seed1": ("ds", lambda s: configured(s, "seed1")),
    "seed2": ("ds", lambda s: configured(s, "seed2")),
    "cold": ("ds", lambda s: configured(s, "cold")),
    "dry": ("ds", lambda s: configured(s, "dry")),
    "moist": ("ds", lambda s: configured(s, "moist")),
    "nssopt0": ("W", lambda s: configured(s, "nssopt0")),
    "nssopt2": ("M", lambda s: configured(s, "nssopt2")),
    "nssopt3": ("M", lambda s: configured(s, "nssopt3")),
    "aerosol_W": ("W", mf.with_aerosols),
    "condensate_x1000": ("ds", lambda s: mf.edge_case(s, "condensate_x1000")),
    "no_water": ("ds", lambda s: mf.edge_case(s, "no_water")),
    "hot_plus60K": ("ds", lambda s: mf.edge_case(s, "hot_plus60K")),
    "cold_minus80K": ("ds", lambda s: mf.edge_case(s, "cold_minus80K")),
    "mass_flux_x100": ("ds", lambda s: mf.edge_case(s, "mass_flux_x100")),
    "ptsphy_7200": ("ds", lambda s: mf.param_case(s, "ptsphy_7200")),
    "tuning_jitter_1": ("ds", lambda s: mf.param_case(s, "tuning_jitter_1")),
    "ncldtop40": ("W", lambda s: _levels_on_w(s, "ncldtop40")),
    "ncldtop138": ("W", lambda s: _levels_on_w(s, "ncldtop138")),
    "klev60": ("W", lambda s: _levels_on_w(s, "klev60")),
    "klev3": ("W", lambda s: _levels_on_w(s, "klev3")),
    "klev274": ("W", lambda s: _levels_on_w(s, "klev274")),
}
STATES = list(BUILDERS)
KLEV_OF = {"klev60": 60, "klev3": 3, "klev274": 274}
# states the oracle is not yet pinned on to the reference kernel elsewhere in tests/test_oracle.py
NEW_FOR_THE_ORACLE = ["aerosol_W", "nssopt0", "nssopt2", "nssopt3", "ncldtop40", "ncldtop138", "klev60", "klev3",
                      "klev274"]

# What the fp64 oracle's outputs must show:
#   "rain"      pfplsl and the rain tendency are both non-zero somewhere
#   "no_rain"   the rain tendency is zero everywhere (the negative controls)
#   "toprfz"    prainfrac_toprfz > 0 in every column
#   "land_sea"  the land mask has columns on both sides of 0.5 (an input property)
# Every state is one or the other of rain / no_rain: the shipped state has no rain at all, and of its
# edges only +60 K makes some; NCLDTOP 138 switches the physics off.
ACTIVITY = {
    "W": {"rain", "land_sea"},
    "M": {"rain", "toprfz", "land_sea"},
    "seed1": {"rain", "land_sea"},
    "seed2": {"rain", "land_sea"},
    "cold": {"no_rain"},
    "dry": {"no_rain"},
    "moist": {"no_rain"},
    "nssopt0": {"rain", "land_sea"},
    "nssopt2": {"rain", "toprfz", "land_sea"},
    "nssopt3": {"rain", "toprfz", "land_sea"},
    "aerosol_W": {"rain", "land_sea"},
    "condensate_x1000": {"no_rain"},
    "no_water": {"no_rain"},
    "hot_plus60K": {"rain"},
    "cold_minus80K": {"no_rain"},
    "mass_flux_x100": {"no_rain"},
    "ptsphy_7200": {"no_rain"},
    "tuning_jitter_1": {"no_rain"},
    "ncldtop40": {"rain", "land_sea"},
    "ncldtop138": {"no_rain", "land_sea"},
    "klev60": {"rain", "land_sea"},
    "klev3": {"rain", "land_sea"},
    "klev274": {"rain", "land_sea"},
}
assert sorted(ACTIVITY) == sorted(BUILDERS)


# the forms' launches on these states (tests/test_forms_states_gpu.py and its tendbuf-outputs companion)
VARIANTS = (ca.VARIANT_KCACHE, ca.VARIANT_KSEG)
TEND_PLANES, ORDER = 11, "permuted"


def shapes(name, packed_form=False):
    if packed_form:
        return [(NGPTOT, 16)] if name == "klev274" else [(NGPTOT, 16), (NGPTOT, 5)]
    return [(NGPTOT, 64), (NGPTOT, 16)]


def schedules(name, variant):
    """(segments, workgroups) of the form's launches: KSEG also with two hand-offs per column."""
    if variant != ca.VARIANT_KSEG or name == "klev3":
        return [(0, 0)]
    return [(0, 0), (3, 3)]


def base_of(name):
    return BUILDERS[name][0]


def rain_active(name):
    return "rain" in ACTIVITY.get(name, ())


_datasets = {}


def dataset(name, ds, scenarios):
    """The state as a Dataset, built once (ds, scenarios: the fixtures of tests/conftest.py)."""
    if name not in _datasets:
        base, build = BUILDERS[name]
        s = build((scenarios[base] if base in scenarios else ds).copy())
        s.reference = {}
        for a in s.inputs.values():
            a.setflags(write=False)
        _datasets[name] = s
    return _datasets[name]


_oracle = {}


def oracle_outputs(oracle_mod, name, s):
    """{field: [..][NGPTOT]} of the fp64 oracle on the state, once per state, read-only."""
    if name not in _oracle:
        st, _ = oracle_mod.run_oracle(s, NGPTOT, ORACLE_NPROMA)
        out = {k: np.ascontiguousarray(ca.blocks_to_columns(st.arrays[k], NGPTOT)) for k in NAMES}
        for a in out.values():
            a.setflags(write=False)
        _oracle[name] = out
    return _oracle[name]


def activity_failures(name, s, out):
    """What of ACTIVITY[name] the oracle's outputs `out` (and the state's inputs) do not show."""
    bad = []
    want = ACTIVITY.get(name, set())
    pfplsl = int(np.count_nonzero(out["pfplsl"]))
    rain = int(np.count_nonzero(out["tendency_loc_cld"][QR]))
    toprfz = int(np.count_nonzero(out["prainfrac_toprfz"] > 0))
    land = int(np.count_nonzero(s.inputs["plsm"] > 0.5))
    if not all(bool(np.all(np.isfinite(a))) for a in out.values()):
        bad.append("non-finite outputs")
    if "rain" in want and not (pfplsl > 0 and rain > 0):
        bad.append("rain: %d non-zero pfplsl, %d non-zero rain tendencies" % (pfplsl, rain))
    if "no_rain" in want and rain != 0:
        bad.append("no_rain: %d non-zero rain tendencies" % rain)
    if "toprfz" in want and toprfz != s.klon:
        bad.append("toprfz: %d of %d columns" % (toprfz, s.klon))
    if "land_sea" in want and not 0 < land < s.klon:
        bad.append("land_sea: %d of %d columns are land" % (land, s.klon))
    return bad
