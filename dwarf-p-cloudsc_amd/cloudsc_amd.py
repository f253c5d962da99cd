"""Host-side mirror of the CLOUDSC dwarf plumbing, over the libcloudsc_amd.so C ABI.

This is the Python face of the same boundary the C host driver
(``dwarf-p-cloudsc_amd/csrc/dwarf_cloudsc_amd.c``) uses.  It mirrors the
reference driver's plumbing:

* dataset loading -- the Serialbox raw arrays + global scalars the reference
  reads (``src/cloudsc_c/cloudsc/load_state.c:279-690``; the ``data/*.dat`` files
  are C-order ``[lev][klon]`` / ``[nclv][lev][klon]`` arrays, exactly the HDF5
  dataset layout of ``config-files/reference.h5``);
* NPROMA-block expansion with the global ``g % klon`` column map
  (``load_state.c:69-184``, ``src/common/module/expand_mod.F90:173-200``);
* field-wise validation with the Fortran ERROR_PRINT semantics
  (``src/common/module/validate_mod.F90:118-296``) -- ``fabs``, not the C
  validator's integer ``abs`` (``cloudsc_validate.c:74,109,147``);
* the GPU state API (device-side expand / run / validate) of ``cloudsc_amd.h``.

The GPU path has no fallback: if ``libcloudsc_amd.so`` is missing or no HIP
device is visible, :func:`gpu_lib` raises.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
LIB_PATH = os.path.join(HERE, "libcloudsc_amd.so")
DATA_DIR = os.path.join(REPO, "data", "cloudsc100")   # the reference's data/ arrays (tools/make_fixtures.py)

NCLV = 5
FP64, FP32 = 8, 4
# float fields, double arithmetic: out == float32(fp64_kernel(float64(in))) bit for bit (cloudsc_amd.h)
MIXED = 12


def storage_dtype(precision: int):
    """Element type of the real fields of a precision code in memory."""
    return np.float64 if precision == FP64 else np.float32
VARIANT_SCC, VARIANT_KCACHE, VARIANT_KSEG, VARIANT_SCC_PRIVATE = 1, 2, 3, 4

# ---------------------------------------------------------------------------
# cloudsc_params_t  (order == include/cloudsc_amd.h)
# ---------------------------------------------------------------------------
PARAM_DOUBLES = (
    "ptsphy rg rd rcpd retv rlvtt rlstt rlmlt rtt rv "
    "r2es r3les r3ies r4les r4ies r5les r5ies r5alvcp r5alscp "
    "ralvdcp ralsdcp ralfdcp rtwat rtice rticecu rtwat_rtice_r rtwat_rticecu_r rkoop1 rkoop2 "
    "ramid rcldiff rcldiff_convi rclcrit rclcrit_sea rclcrit_land rkconv rprc1 rprc2 "
    "rcldmax rpecons rvrfactor rprecrhmax rtaumel ramin rlmin rkooptau rcldtopp "
    "rlcritsnow rsnowlin1 rsnowlin2 ricehi1 ricehi2 riceinit rvice rvrain rvsnow "
    "rthomo rcovpmin rccn rnice rccnom rccnss rccnsu rcldtopcf rdepliqrefrate "
    "rdepliqrefdepth rcl_kkaac rcl_kkbac rcl_kkaau rcl_kkbauq rcl_kkbaun "
    "rcl_kk_cloud_num_sea rcl_kk_cloud_num_land rcl_ai rcl_bi rcl_ci rcl_di "
    "rcl_x1i rcl_x2i rcl_x3i rcl_x4i rcl_const1i rcl_const2i rcl_const3i rcl_const4i "
    "rcl_const5i rcl_const6i rcl_apb1 rcl_apb2 rcl_apb3 rcl_as rcl_bs rcl_cs rcl_ds "
    "rcl_x1s rcl_x2s rcl_x3s rcl_x4s rcl_const1s rcl_const2s rcl_const3s rcl_const4s "
    "rcl_const5s rcl_const6s rcl_const7s rcl_const8s rdenswat rdensref rcl_ar rcl_br "
    "rcl_cr rcl_dr rcl_x1r rcl_x2r rcl_x4r rcl_ka273 rcl_cdenom1 rcl_cdenom2 rcl_cdenom3 "
    "rcl_schmidt rcl_dynvisc rcl_const1r rcl_const2r rcl_const3r rcl_const4r rcl_fac1 "
    "rcl_fac2 rcl_const5r rcl_const6r rcl_fzrab rcl_fzrbb nshapep nshapeq"
).split()
PARAM_INTS = (
    "lcldextra lcldbudget nssopt ncldtop naeclbc naecldu naeclom naeclss naeclsu nclddiag "
    "naercld laerliqautolsp laerliqautocp laerliqautocpb laerliqcoll laericesed laericeauto nbeta"
).split()


class Params(C.Structure):
    _fields_ = [(n, C.c_double) for n in PARAM_DOUBLES] + [(n, C.c_int) for n in PARAM_INTS]

    @classmethod
    def from_dict(cls, d: Dict[str, float]) -> "Params":
        p = cls()
        for n in PARAM_DOUBLES:
            setattr(p, n, float(d[n]))
        for n in PARAM_INTS:
            setattr(p, n, int(d[n]))
        return p

    def to_dict(self) -> Dict[str, float]:
        return {n: getattr(self, n) for n in PARAM_DOUBLES + PARAM_INTS}


# ---------------------------------------------------------------------------
# field inventory
# ---------------------------------------------------------------------------
# One (member, kind, direction) row per cloudsc_fields_t member, in member order: csrc/cloudsc_fields.def in
# Python (tests/test_field_inventory.py holds the two together).
# kind: "2d" [lev][klon], "2dh" [lev+1][klon], "3d" [nclv][lev][klon], "1d" [klon]
FIELD_INVENTORY = [
    ("pt", "2d", "in"), ("pq", "2d", "in"), ("tendency_tmp_t", "2d", "in"), ("tendency_tmp_q", "2d", "in"),
    ("tendency_tmp_a", "2d", "in"), ("tendency_tmp_cld", "3d", "in"), ("pvfl", "2d", "in"), ("pvfi", "2d", "in"),
    ("phrsw", "2d", "in"), ("phrlw", "2d", "in"), ("pvervel", "2d", "in"), ("pap", "2d", "in"), ("paph", "2dh", "in"),
    ("plsm", "1d", "in"), ("ktype", "1d", "in"), ("plu", "2d", "in"), ("psnde", "2d", "in"), ("pmfu", "2d", "in"),
    ("pmfd", "2d", "in"), ("pa", "2d", "in"), ("pclv", "3d", "in"), ("psupsat", "2d", "in"),
    ("plcrit_aer", "2d", "aerosol"), ("picrit_aer", "2d", "aerosol"), ("pre_ice", "2d", "aerosol"),
    ("pccn", "2d", "aerosol"), ("pnice", "2d", "aerosol"), ("plude", "2d", "inout"), ("tendency_loc_t", "2d", "out"),
    ("tendency_loc_q", "2d", "out"), ("tendency_loc_a", "2d", "out"), ("tendency_loc_cld", "3d", "out"),
    ("pcovptot", "2d", "out"), ("prainfrac_toprfz", "1d", "out"), ("pfsqlf", "2dh", "out"), ("pfsqif", "2dh", "out"),
    ("pfcqnng", "2dh", "out"), ("pfcqlng", "2dh", "out"), ("pfsqrf", "2dh", "out"), ("pfsqsf", "2dh", "out"),
    ("pfcqrng", "2dh", "out"), ("pfcqsng", "2dh", "out"), ("pfsqltur", "2dh", "out"), ("pfsqitur", "2dh", "out"),
    ("pfplsl", "2dh", "out"), ("pfplsn", "2dh", "out"), ("pfhpsl", "2dh", "out"), ("pfhpsn", "2dh", "out"),
]
INPUT_FIELDS, AEROSOL_FIELDS, INOUT_FIELDS, OUTPUT_FIELDS = (
    {n: k for n, k, d in FIELD_INVENTORY if d == direction} for direction in ("in", "aerosol", "inout", "out"))
ALL_FIELDS = {n: k for n, k, _ in FIELD_INVENTORY}

# The 21 validated fields in the dwarf's print order (cloudsc_validate.c:193-216).
VALIDATED = [
    ("PLUDE", "plude"), ("PCOVPTOT", "pcovptot"), ("PRAINFRAC_TOPRFZ", "prainfrac_toprfz"),
    ("PFSQLF", "pfsqlf"), ("PFSQIF", "pfsqif"), ("PFCQLNG", "pfcqlng"), ("PFCQNNG", "pfcqnng"),
    ("PFSQRF", "pfsqrf"), ("PFSQSF", "pfsqsf"), ("PFCQRNG", "pfcqrng"), ("PFCQSNG", "pfcqsng"),
    ("PFSQLTUR", "pfsqltur"), ("PFSQITUR", "pfsqitur"), ("PFPLSL", "pfplsl"), ("PFPLSN", "pfplsn"),
    ("PFHPSL", "pfhpsl"), ("PFHPSN", "pfhpsn"), ("TENDENCY_LOC%A", "tendency_loc_a"),
    ("TENDENCY_LOC%Q", "tendency_loc_q"), ("TENDENCY_LOC%T", "tendency_loc_t"),
    ("TENDENCY_LOC%CLD", "tendency_loc_cld"),
]
# Fortran NDIM printed by ERROR_PRINT (VALIDATE_R1/R2/R3)
VALIDATED_NDIM = {n: (1 if ALL_FIELDS[k] == "1d" else 3 if ALL_FIELDS[k] == "3d" else 2) for n, k in VALIDATED}


class Fields(C.Structure):
    """cloudsc_fields_t (pointer order == include/cloudsc_amd.h)."""
    _fields_ = [(n, C.c_void_p) for n in ALL_FIELDS]


class LevelsFields(Fields):
    """The Fields of a LAYOUT_LEVELS set (DeviceFields(layout=LAYOUT_LEVELS)): the same struct, marked so that
    the step wrappers can refuse it -- only convert_fields_layout takes such a set."""


def require_blocked(f, what: str) -> None:
    if isinstance(f, LevelsFields):
        raise ValueError("%s takes a block-layout field set; this one is LAYOUT_LEVELS: convert it first "
                         "(convert_fields_layout / DeviceFields.convert_to)" % what)


class TendCml(C.Structure):
    """cloudsc_tend_cml_t: the plane starts of the cumulative tendency buffer (BUFFER_CML) in block 0; cld
    is the first of five consecutive planes, the fifth (vapour) never touched."""
    _fields_ = [(n, C.c_void_p) for n in ("t", "q", "a", "cld")]


SPP_SLOTS = ("ramid", "rcldiff", "rclcrit", "rlcritsnow", "rpecons")


class Spp(C.Structure):
    """cloudsc_spp_t: per-column parameter multipliers, each a surface field [nblocks][nproma] in the storage
    type (the layout of plsm), or None where the parameter is not perturbed."""
    _fields_ = [(n, C.c_void_p) for n in SPP_SLOTS]


class Advance(C.Structure):
    """cloudsc_advance_t: where an advancing step stores the updated prognostics -- t, q, a [nblocks][klev][nproma]
    and clv [nblocks][5][klev][nproma] (the vapour plane never written) in the set's storage type.  Each is the
    set's own pt / pq / pa / pclv (in place) or another array."""
    _fields_ = [(n, C.c_void_p) for n in ("t", "q", "a", "clv")]

    @classmethod
    def in_place(cls, f: "Fields") -> "Advance":
        """The Advance that rewrites pt, pq, pa and pclv of f."""
        return cls(f.pt, f.pq, f.pa, f.pclv)


class Placement(C.Structure):
    """cloudsc_placement_t: what a placement search cost and found."""
    _fields_ = [("probe_first_ms", C.c_float), ("probe_final_ms", C.c_float), ("tries", C.c_int),
                ("moves", C.c_int), ("launches", C.c_int), ("method", C.c_int), ("search_ms", C.c_double),
                ("peak_transient_bytes", C.c_longlong), ("transient_budget_bytes", C.c_longlong)]

    def to_dict(self) -> dict:
        return {"probe_first_ms": round(self.probe_first_ms, 4), "probe_final_ms": round(self.probe_final_ms, 4),
                "tries": self.tries, "moves": self.moves, "launches": self.launches,
                "method": {0: "none", 1: "kernel", 2: "write-probe", 3: "rw-probe"}.get(self.method, self.method),
                "search_ms": round(self.search_ms, 1), "peak_transient_bytes": self.peak_transient_bytes,
                "transient_budget_bytes": self.transient_budget_bytes}


PLACE_NONE = 1
ALLOC_AEROSOLS = 2
# output selection (cloudsc_gpu_run_outputs, cloudsc_cpu_run_outputs, cloudsc_fields_alloc_outputs)
# (a bit set: bit 0 = no diagnostic flux profiles, bit 2 = the four precipitation / enthalpy fluxes at the
# surface only, valid with bit 0 alone; 2, 4 and every other value are unknown)
OUTPUTS_ALL, OUTPUTS_PROGNOSTIC, OUTPUTS_SURFACE = 0, 1, 5
# the ten diagnostic flux outputs OUTPUTS_PROGNOSTIC leaves out: the running sums of section 8
DIAGNOSTIC_FLUX_FIELDS = ("pfsqlf", "pfsqif", "pfcqnng", "pfcqlng", "pfsqrf", "pfsqsf", "pfcqrng", "pfcqsng",
                          "pfsqltur", "pfsqitur")
# the four flux outputs OUTPUTS_SURFACE keeps as surface fields [nblocks][nproma]: row klev of their profiles
SURFACE_FLUX_FIELDS = ("pfplsl", "pfplsn", "pfhpsl", "pfhpsn")
# field set layouts (cloudsc_fields_convert_layout): [nblocks][rows][nproma], what every step takes, and
# [ngptot][rows], the rows of one column contiguous
LAYOUT_BLOCKED, LAYOUT_LEVELS = 0, 1


def selected_outputs(outputs: int = OUTPUTS_ALL) -> tuple:
    """The output members (plude included) an output selection writes, in member order: all 21, or the
    eleven OUTPUTS_PROGNOSTIC and OUTPUTS_SURFACE keep (selected_field_shape has their shapes)."""
    if outputs not in (OUTPUTS_ALL, OUTPUTS_PROGNOSTIC, OUTPUTS_SURFACE):
        raise ValueError("unknown output selection: %r" % (outputs,))
    return tuple(n for n in list(INOUT_FIELDS) + list(OUTPUT_FIELDS)
                 if outputs == OUTPUTS_ALL or n not in DIAGNOSTIC_FLUX_FIELDS)


def selected_field_shape(name: str, klev: int, klon: int, outputs: int = OUTPUTS_ALL) -> tuple:
    """The per-block shape of member `name` under an output selection: field_shape of its kind, except that
    OUTPUTS_SURFACE holds the SURFACE_FLUX_FIELDS as surface fields, (klon,)."""
    if outputs not in (OUTPUTS_ALL, OUTPUTS_PROGNOSTIC, OUTPUTS_SURFACE):
        raise ValueError("unknown output selection: %r" % (outputs,))
    if name not in ALL_FIELDS:
        raise KeyError("no such field: %s" % name)
    if outputs == OUTPUTS_SURFACE and name in SURFACE_FLUX_FIELDS:
        return (klon,)
    return field_shape(ALL_FIELDS[name], klev, klon)


class LaunchGeometry(C.Structure):
    """cloudsc_launch_geometry_t: what a physics launch would look like."""
    _fields_ = [("pack", C.c_int), ("lanes", C.c_int), ("units", C.c_int), ("workgroups", C.c_int),
                ("wg_threads", C.c_int)]

    def to_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


TEMPLATE_ORDER = list(INPUT_FIELDS)
TEMPLATE_ORDER.insert(TEMPLATE_ORDER.index("plu") + 1, "plude")   # where the reference's files have it
TEMPLATE_ORDER += AEROSOL_FIELDS


class Template(C.Structure):
    _fields_ = [("klon", C.c_int), ("klev", C.c_int)] + [(n, C.c_void_p) for n in TEMPLATE_ORDER]


class Reference(C.Structure):
    _fields_ = [("klon", C.c_int), ("klev", C.c_int), ("field", C.c_void_p * 21)]


class Stats(C.Structure):
    _fields_ = [("minval", C.c_double), ("maxval", C.c_double), ("maxerr", C.c_double),
                ("errsum", C.c_double), ("refsum", C.c_double),
                ("errsum_lo", C.c_double), ("refsum_lo", C.c_double)]


class FieldDiff(C.Structure):
    """cloudsc_field_diff_t: one member of a field set against the same member of another."""
    _fields_ = [("stats", Stats), ("compared", C.c_longlong), ("mismatches", C.c_longlong),
                ("first_column", C.c_longlong), ("first_row", C.c_longlong)]

    def to_dict(self) -> dict:
        s = self.stats
        return {"stats": (s.minval, s.maxval, s.maxerr, s.errsum, s.refsum, s.errsum_lo, s.refsum_lo),
                "compared": self.compared, "mismatches": self.mismatches,
                "first": (self.first_column, self.first_row) if self.mismatches else None}


# ---------------------------------------------------------------------------
# dataset (template) I/O
# ---------------------------------------------------------------------------
def field_shape(kind: str, klev: int, klon: int):
    return {"2d": (klev, klon), "2dh": (klev + 1, klon), "3d": (NCLV, klev, klon), "1d": (klon,)}[kind]


def read_params_txt(path: str) -> Dict[str, float]:
    out: Dict[str, float] = {}
    with open(path) as fh:
        for line in fh:
            line = line.split("#", 1)[0].strip()
            if not line:
                continue
            name, val = line.split("=")
            name, val = name.strip(), val.strip()
            out[name] = int(val) if name in PARAM_INTS else float(val)
    return out


def write_params_txt(path: str, params: Dict[str, float]) -> None:
    with open(path, "w") as fh:
        fh.write("# CLOUDSC parameter block (YOMCST, YOETHF, TECLDP, PTSPHY); %.17g = exact\n")
        for n in PARAM_DOUBLES:
            fh.write("%s = %.17g\n" % (n, params[n]))
        for n in PARAM_INTS:
            fh.write("%s = %d\n" % (n, int(params[n])))


@dataclass
class Dataset:
    """KLON template columns + parameters (+ optional reference outputs)."""
    klon: int
    klev: int
    params: Dict[str, float]
    inputs: Dict[str, np.ndarray]
    reference: Dict[str, np.ndarray] = field(default_factory=dict)

    def copy(self) -> "Dataset":
        return Dataset(self.klon, self.klev, dict(self.params),
                       {k: v.copy() for k, v in self.inputs.items()},
                       {k: v.copy() for k, v in self.reference.items()})


def read_serialbox_params(path: str) -> Dict[str, float]:
    """The parameter block from a Serialbox store's MetaData-input.json
    (global_meta_info, the input.h5 scalar names: RG, ..., YRECLDP_<NAME>;
    logicals as 0/1), keyed like params.txt (lower case, no YRECLDP_ prefix)."""
    g = json.load(open(os.path.join(path, "MetaData-input.json")))["global_meta_info"]
    by_key = {}
    for name, v in g.items():
        key = (name[8:] if name.startswith("YRECLDP_") else name).lower()
        by_key[key] = v["value"]
    out: Dict[str, float] = {}
    for n in PARAM_DOUBLES:
        out[n] = float(by_key[n])
    for n in PARAM_INTS:
        out[n] = int(by_key[n])
    return out


def load_dataset(path: str = DATA_DIR, with_reference: bool = True) -> Dataset:
    """Read a data directory: a Serialbox store (the reference's data/:
    MetaData-input.json + input_<NAME>.dat, reference_<NAME>.dat) or the raw
    form written by tools/make_fixtures.py (manifest.json + params.txt + the
    same .dat arrays)."""
    if os.path.exists(os.path.join(path, "MetaData-input.json")):
        g = json.load(open(os.path.join(path, "MetaData-input.json")))["global_meta_info"]
        klon, klev = int(g["KLON"]["value"]), int(g["KLEV"]["value"])
        params = read_serialbox_params(path)
    else:
        man = json.load(open(os.path.join(path, "manifest.json")))
        klon, klev = man["klon"], man["klev"]
        params = read_params_txt(os.path.join(path, "params.txt"))
    inputs = {}
    for name, kind in {**INPUT_FIELDS, **AEROSOL_FIELDS, **INOUT_FIELDS}.items():
        fn = os.path.join(path, "input_%s.dat" % name.upper())
        if not os.path.exists(fn):
            continue
        dt = np.int32 if name == "ktype" else np.float64
        inputs[name] = np.fromfile(fn, dtype=dt).reshape(field_shape(kind, klev, klon))
    ref = {}
    if with_reference:
        for vname, key in VALIDATED:
            fn = os.path.join(path, "reference_%s.dat" % key.upper())
            if os.path.exists(fn):
                ref[key] = np.fromfile(fn, dtype=np.float64).reshape(field_shape(ALL_FIELDS[key], klev, klon))
    return Dataset(klon, klev, params, inputs, ref)


# ---------------------------------------------------------------------------
# NPROMA-block expansion / contraction (host, numpy)
# ---------------------------------------------------------------------------
def nblocks_of(ngptot: int, nproma: int) -> int:
    return ngptot // nproma + (1 if ngptot % nproma else 0)


def global_columns(ngptot: int, nproma: int, col_offset: int = 0) -> np.ndarray:
    """[nblocks, nproma] global column index of every block lane (lanes past
    ngptot replicate the map, like the C loader's expand_* which fills them)."""
    nb = nblocks_of(ngptot, nproma)
    return col_offset + np.arange(nb * nproma, dtype=np.int64).reshape(nb, nproma)


def expand(arr: np.ndarray, kind: str, ngptot: int, nproma: int, col_offset: int = 0,
           dtype=None) -> np.ndarray:
    """Template ``[..][klon]`` -> block layout ``[nblocks][..][nproma]`` with g % klon."""
    klon = arr.shape[-1]
    src = global_columns(ngptot, nproma, col_offset) % klon            # [nb, nproma]
    out = np.take(arr, src, axis=-1)                                   # [..., nb, nproma]
    out = np.moveaxis(out, -2, 0)                                      # [nb, ..., nproma]
    return np.ascontiguousarray(out, dtype=dtype or arr.dtype)


def blocks_to_columns(arr: np.ndarray, ngptot: int) -> np.ndarray:
    """Block layout ``[nb][..][nproma]`` -> column-last ``[..][ngptot]``."""
    x = np.moveaxis(arr, 0, -2)                                        # [..., nb, nproma]
    x = x.reshape(x.shape[:-2] + (-1,))
    return x[..., :ngptot]


@dataclass
class HostState:
    """All kernel fields in block layout on the host (used with the oracle)."""
    ngptot: int
    nproma: int
    klev: int
    precision: int
    arrays: Dict[str, np.ndarray]

    def fields(self) -> Fields:
        f = Fields()
        for name, _ in Fields._fields_:
            a = self.arrays.get(name)
            setattr(f, name, a.ctypes.data if a is not None else None)
        return f


_KIND_CODE = {"2d": 0, "2dh": 1, "3d": 2, "1d": 3}
_io = None


def io_lib():
    """libcloudsc_io.so (host-only dataset plumbing of the C driver), or None if
    it is not built -- then the numpy forms below are used (same results)."""
    global _io
    if _io is None:
        path = os.path.join(HERE, "libcloudsc_io.so")
        if not os.path.exists(path):
            return None
        lib = C.CDLL(path)
        lib.cloudsc_io_expand.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_longlong, C.c_int, C.c_void_p]
        lib.cloudsc_io_field_stats.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                               C.c_int, C.c_int, C.c_longlong, C.c_void_p]
        _io = lib
    return _io


def make_host_state(ds: Dataset, ngptot: int, nproma: int, precision: int = FP64,
                    col_offset: int = 0) -> HostState:
    real = storage_dtype(precision)
    nb = nblocks_of(ngptot, nproma)
    arrays = {}
    io = io_lib()
    for name, arr in ds.inputs.items():
        kind = ALL_FIELDS[name]
        dt = np.int32 if name == "ktype" else real
        if io is not None and arr.dtype == (np.int32 if name == "ktype" else np.float64):
            src = np.ascontiguousarray(arr)
            out = np.empty((nb,) + field_shape(kind, ds.klev, nproma), dtype=dt)
            io.cloudsc_io_expand(src.ctypes.data, _KIND_CODE[kind], int(name == "ktype"), ds.klev, ds.klon,
                                 ngptot, nproma, col_offset, out.itemsize, out.ctypes.data)
            arrays[name] = out
        else:
            arrays[name] = expand(arr, kind, ngptot, nproma, col_offset, dtype=dt)
    for name, kind in OUTPUT_FIELDS.items():
        shp = (nb,) + field_shape(kind, ds.klev, nproma)
        arrays[name] = np.full(shp, np.nan, dtype=real)                # callee must write all
    return HostState(ngptot, nproma, ds.klev, precision, arrays)


# ---------------------------------------------------------------------------
# validation (Fortran ERROR_PRINT semantics, validate_mod.F90:118-296)
# ---------------------------------------------------------------------------
def field_stats(field: np.ndarray, ref: np.ndarray) -> tuple:
    f = field.astype(np.float64).ravel()
    r = ref.astype(np.float64).ravel()
    d = np.abs(f - r)
    return (float(f.min()), float(f.max()), float(d.max()), float(d.sum()), float(np.abs(r).sum()))


def rel_error(errsum: float, refsum: float, eps: float = np.finfo(np.float64).eps):
    """(zrelerr, iopt) exactly as ERROR_PRINT (validate_mod.F90:273-283)."""
    if errsum < eps:
        return 0.0, 1
    if refsum < eps:
        return errsum / (1.0 + refsum), 2
    return errsum / refsum, 3


def format_row(name: str, ndim: int, st: tuple, ngptot: int, eps: float = np.finfo(np.float64).eps) -> str:
    mn, mx, maxerr, errsum, refsum = st
    rel, iopt = rel_error(errsum, refsum, eps)
    warn = " !!!!" if rel > 10.0 * eps else "     "
    # Fortran format (1X,A20,1X,I1,'D',I1,5(1X,E20.13),A)
    return " %20s %dD%d %20.13E %20.13E %20.13E %20.13E %20.13E%s" % (
        name, ndim, iopt, mn, mx, maxerr, errsum / ngptot, 100.0 * rel, warn)


def state_outputs_to_template(arrays: Dict[str, np.ndarray], ngptot: int) -> Dict[str, np.ndarray]:
    return {k: blocks_to_columns(arrays[k], ngptot) for _, k in VALIDATED}


# ---------------------------------------------------------------------------
# GPU library (no fallback)
# ---------------------------------------------------------------------------
class CloudscError(RuntimeError):
    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


_lib = None


def gpu_lib(path: Optional[str] = None):
    """Load libcloudsc_amd.so.  Raises if it is missing: there is no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("CLOUDSC_AMD_LIB", LIB_PATH)
    if not os.path.exists(path):
        raise CloudscError("libcloudsc_amd.so not built (%s): run __graft_entry__.build()" % path)
    lib = C.CDLL(path)
    lib.cloudsc_strerror.restype = C.c_char_p
    lib.cloudsc_last_hip_error.restype = C.c_char_p
    lib.cloudsc_abi_sizeof.restype = C.c_longlong
    lib.cloudsc_gpu_scratch_bytes.restype = C.c_longlong
    lib.cloudsc_state_field_elems.restype = C.c_longlong
    lib.cloudsc_state_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_longlong, C.POINTER(Template), C.POINTER(Params)]
    lib.cloudsc_state_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]
    lib.cloudsc_state_run_span.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]
    lib.cloudsc_state_validate.argtypes = [C.c_void_p, C.POINTER(Reference), C.POINTER(Stats)]
    lib.cloudsc_state_download.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.cloudsc_state_field_elems.argtypes = [C.c_void_p, C.c_int]
    lib.cloudsc_state_destroy.argtypes = [C.c_void_p]
    lib.cloudsc_state_sync.argtypes = [C.c_void_p]
    lib.cloudsc_state_reset.argtypes = [C.c_void_p]
    lib.cloudsc_state_fields.argtypes = [C.c_void_p, C.POINTER(Fields)]
    if hasattr(lib, "cloudsc_state_placement"):
        lib.cloudsc_state_placement.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.cloudsc_debug_set_placement_search.argtypes = [C.c_int]
    if hasattr(lib, "cloudsc_debug_set_pipeline_copy"):
        lib.cloudsc_debug_set_pipeline_copy.argtypes = [C.c_int]
        lib.cloudsc_debug_host_pipeline_copy.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                                         C.POINTER(C.c_int)]
        lib.cloudsc_debug_host_pipeline_engine_check.argtypes = [C.c_void_p, C.POINTER(C.c_double),
                                                                 C.POINTER(C.c_int)]
        lib.cloudsc_host_pipeline_copy_bound.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    if hasattr(lib, "cloudsc_debug_memory_probe"):
        lib.cloudsc_debug_memory_probe.argtypes = [C.c_int] * 5 + [C.POINTER(Fields), C.c_int, C.c_int,
                                                                  C.POINTER(C.c_float)]
    if hasattr(lib, "cloudsc_fields_alloc"):
        lib.cloudsc_fields_alloc.argtypes = [C.c_int] * 6 + [C.POINTER(Fields), C.POINTER(Placement)]
        lib.cloudsc_fields_free.argtypes = [C.c_int, C.POINTER(Fields)]
        lib.cloudsc_state_placement_report.argtypes = [C.c_void_p, C.POINTER(Placement)]
    lib.cloudsc_gpu_init.argtypes = [C.c_int, C.POINTER(Params)]
    lib.cloudsc_gpu_run.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.POINTER(Fields), C.c_void_p]
    lib.cloudsc_host_pipeline_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int,
                                                 C.c_int, C.c_int, C.c_int, C.POINTER(Fields)]
    lib.cloudsc_host_pipeline_run.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    lib.cloudsc_host_pipeline_destroy.argtypes = [C.c_void_p]
    lib.cloudsc_gpu_check.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.cloudsc_hbm_copy_gbps.argtypes = [C.c_int, C.c_longlong, C.c_int, C.POINTER(C.c_double)]
    if hasattr(lib, "cloudsc_pcie_gbps"):   # (older experiment builds lack it)
        lib.cloudsc_pcie_gbps.argtypes = [C.c_int, C.c_longlong, C.c_int] + [C.POINTER(C.c_double)] * 3
    lib.cloudsc_cpu_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Params), C.POINTER(Fields),
                                    C.POINTER(C.c_double)]
    lib.cloudsc_cpu_run_precision.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Params),
                                              C.POINTER(Fields), C.POINTER(C.c_double)]
    # (device, stream | nthreads), ngptot, klev, then precision, nproma, fields of src and of dst
    lib.cloudsc_fields_convert.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Fields),
                                           C.c_int, C.c_int, C.POINTER(Fields)]
    lib.cloudsc_cpu_fields_convert.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Fields),
                                               C.c_int, C.c_int, C.POINTER(Fields)]
    # the same argument order, then one FieldDiff per Fields member
    lib.cloudsc_tendbuf_bind.argtypes = [C.POINTER(Fields), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.cloudsc_gpu_run_tendbuf.argtypes = [C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.POINTER(Fields), C.c_void_p]
    lib.cloudsc_cpu_run_tendbuf.argtypes = [C.c_int] * 6 + [C.POINTER(Params), C.POINTER(Fields)]
    lib.cloudsc_fields_convert_tendbuf.argtypes = [C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.POINTER(Fields)] + \
        [C.c_int] * 3 + [C.POINTER(Fields)]
    lib.cloudsc_cpu_fields_convert_tendbuf.argtypes = [C.c_int] * 6 + [C.POINTER(Fields)] + [C.c_int] * 3 + \
        [C.POINTER(Fields)]
    lib.cloudsc_gpu_run_outputs.argtypes = [C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.POINTER(Fields), C.c_void_p]
    lib.cloudsc_cpu_run_outputs.argtypes = [C.c_int] * 6 + [C.POINTER(Params), C.POINTER(Fields)]
    lib.cloudsc_fields_alloc_outputs.argtypes = [C.c_int] * 7 + [C.POINTER(Fields), C.POINTER(Placement)]
    lib.cloudsc_fields_compare.argtypes = lib.cloudsc_fields_convert.argtypes + [C.POINTER(FieldDiff)]
    lib.cloudsc_cpu_fields_compare.argtypes = lib.cloudsc_cpu_fields_convert.argtypes + [C.POINTER(FieldDiff)]
    lib.cloudsc_fields_validate.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong,
                                            C.POINTER(Fields), C.POINTER(Reference), C.POINTER(Stats)]
    lib.cloudsc_fields_expand.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_longlong,
                                          C.POINTER(Template), C.POINTER(Fields)]
    # the tendency buffers with an output selection, and compare / validate / expand on them in place
    if hasattr(lib, "cloudsc_gpu_run_tendbuf_outputs"):   # (an older library under CLOUDSC_AMD_LIB, for A/B runs, lacks them)
        lib.cloudsc_gpu_run_tendbuf_outputs.argtypes = [C.c_int, C.c_void_p] + [C.c_int] * 7 + [C.POINTER(Fields),
                                                                                                 C.c_void_p]
        lib.cloudsc_cpu_run_tendbuf_outputs.argtypes = [C.c_int] * 7 + [C.POINTER(Params), C.POINTER(Fields)]
        lib.cloudsc_fields_compare_tendbuf.argtypes = lib.cloudsc_fields_convert_tendbuf.argtypes + \
            [C.POINTER(FieldDiff)]
        lib.cloudsc_cpu_fields_compare_tendbuf.argtypes = lib.cloudsc_cpu_fields_convert_tendbuf.argtypes + \
            [C.POINTER(FieldDiff)]
        lib.cloudsc_fields_validate_tendbuf.argtypes = [C.c_int, C.c_void_p] + [C.c_int] * 6 + [
            C.c_longlong, C.POINTER(Fields), C.POINTER(Reference), C.POINTER(Stats)]
        lib.cloudsc_fields_expand_tendbuf.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                      C.c_longlong, C.POINTER(Template), C.POINTER(Fields)]
    if hasattr(lib, "cloudsc_gpu_run_tendbuf_cml"):   # (likewise: the cumulative tendency buffer)
        lib.cloudsc_tendbuf_bind_cml.argtypes = [C.POINTER(TendCml), C.c_int, C.c_int, C.c_int, C.c_void_p]
        lib.cloudsc_gpu_run_tendbuf_cml.argtypes = [C.c_int, C.c_void_p] + [C.c_int] * 7 + [
            C.POINTER(Fields), C.POINTER(TendCml), C.c_void_p]
        lib.cloudsc_cpu_run_tendbuf_cml.argtypes = [C.c_int] * 7 + [C.POINTER(Params), C.POINTER(Fields),
                                                                    C.POINTER(TendCml)]
        lib.cloudsc_fields_accumulate_tendbuf.argtypes = [C.c_int, C.c_void_p] + [C.c_int] * 5 + [
            C.POINTER(Fields), C.c_int, C.POINTER(TendCml)]
        lib.cloudsc_cpu_fields_accumulate_tendbuf.argtypes = [C.c_int] * 6 + [C.POINTER(Fields), C.c_int,
                                                                              C.POINTER(TendCml)]
    if hasattr(lib, "cloudsc_gpu_run_spp"):   # (likewise: the per-column parameter multipliers)
        lib.cloudsc_gpu_run_spp.argtypes = [C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.POINTER(Fields), C.POINTER(Spp),
                                                                                    C.c_void_p]
        lib.cloudsc_cpu_run_spp.argtypes = [C.c_int] * 6 + [C.POINTER(Params), C.POINTER(Fields), C.POINTER(Spp)]
    if hasattr(lib, "cloudsc_gpu_run_advance"):   # (likewise: the advancing step and its separate pass)
        lib.cloudsc_gpu_run_advance.argtypes = [C.c_int, C.c_void_p] + [C.c_int] * 6 + [
            C.POINTER(Fields), C.POINTER(Advance), C.c_void_p]
        lib.cloudsc_cpu_run_advance.argtypes = [C.c_int] * 6 + [C.POINTER(Params), C.POINTER(Fields),
                                                                C.POINTER(Advance)]
        lib.cloudsc_fields_advance.argtypes = [C.c_int, C.c_void_p] + [C.c_int] * 4 + [C.POINTER(Fields),
                                                                                       C.POINTER(Advance)]
        lib.cloudsc_cpu_fields_advance.argtypes = [C.c_int] * 5 + [C.POINTER(Params), C.POINTER(Fields),
                                                                   C.POINTER(Advance)]
    if hasattr(lib, "cloudsc_fields_compare_outputs"):   # (likewise: the forms for a set of one output selection)
        lib.cloudsc_fields_convert_outputs.argtypes = [C.c_int, C.c_void_p] + [C.c_int] * 5 + [
            C.POINTER(Fields), C.c_int, C.c_int, C.POINTER(Fields)]
        lib.cloudsc_fields_compare_outputs.argtypes = lib.cloudsc_fields_convert_outputs.argtypes + \
            [C.POINTER(FieldDiff)]
    if hasattr(lib, "cloudsc_fields_convert_layout"):   # (likewise: the layout conversion)
        # (device, stream | nthreads), ngptot, klev, outputs, then precision, layout, nproma, fields of src and of dst
        lib.cloudsc_fields_convert_layout.argtypes = [C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.POINTER(Fields)] + \
            [C.c_int] * 3 + [C.POINTER(Fields)]
        lib.cloudsc_cpu_fields_convert_layout.argtypes = [C.c_int] * 7 + [C.POINTER(Fields)] + [C.c_int] * 3 + \
            [C.POINTER(Fields)]
    lib.cloudsc_fields_diff_sizeof.restype = C.c_longlong
    lib.cloudsc_fields_compare_release.argtypes = [C.c_int]
    lib.cloudsc_debug_set_compare_grid.argtypes = [C.c_int]
    if (lib.cloudsc_fields_diff_sizeof() != C.sizeof(FieldDiff)
            or lib.cloudsc_fields_members() != len(Fields._fields_)):
        raise CloudscError("FieldDiff / Fields do not match libcloudsc_amd.so (cloudsc_field_diff_t)")
    lib.cloudsc_debug_set_kseg_spin_limit.argtypes = [C.c_longlong]
    lib.cloudsc_debug_set_kseg_schedule.argtypes = [C.c_int, C.c_int]
    lib.cloudsc_gpu_launch_geometry.argtypes = [C.c_int] * 6 + [C.POINTER(LaunchGeometry)]
    lib.cloudsc_debug_set_narrow_pack.argtypes = [C.c_int]
    if hasattr(lib, "cloudsc_batch_create"):   # (likewise: the batched step)
        # batch, device, precision, outputs, nsets, ngptot, nproma, klev, sets[nsets], params[nsets] or NULL
        lib.cloudsc_batch_create.argtypes = [C.POINTER(C.c_void_p)] + [C.c_int] * 7 + [C.POINTER(Fields),
                                                                                      C.POINTER(Params)]
        lib.cloudsc_gpu_run_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.cloudsc_batch_nsets.argtypes = [C.c_void_p]
        lib.cloudsc_batch_destroy.argtypes = [C.c_void_p]
        lib.cloudsc_batch_launch_geometry.argtypes = [C.c_int] * 6 + [C.POINTER(LaunchGeometry)]
    lib.cloudsc_debug_host_pipeline_mapping.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.cloudsc_debug_host_pinned.argtypes = [C.c_void_p, C.c_longlong]
    lib.cloudsc_debug_fp32_libm.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]
    lib.cloudsc_debug_fp64_libm.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_longlong]
    _lib = lib
    return lib


EINVAL = -1
EHANDOFF = -7
# option bit of a variant argument: fp32 exp/pow with the glibc algorithms (bit-identical to the fp32 restatement)
FP32_EXACT_LIBM = 0x100


def kseg_schedule(nseg: int = 0, grid: int = 0) -> None:
    """Diagnostic override of the KSEG schedule (0 = default); results do not change."""
    check(gpu_lib().cloudsc_debug_set_kseg_schedule(nseg, grid))


def narrow_pack(mode: int = -1) -> None:
    """Process-wide: 1 = run blocks of NPROMA <= 32 packed, 64 // nproma blocks per wave (KCACHE, KSEG),
    0 = never, negative = the measured default per width.  The result bits do not depend on it."""
    check(gpu_lib().cloudsc_debug_set_narrow_pack(mode))


def launch_geometry(precision: int, variant: int, ngptot: int, nproma: int, klev: int, laer: bool = False) -> dict:
    """What cloudsc_gpu_run would launch for these arguments (pack, lanes, units, workgroups, wg_threads);
    host arithmetic, no GPU needed.  Raises CloudscError (code EINVAL) as the run would."""
    g = LaunchGeometry()
    check(gpu_lib().cloudsc_gpu_launch_geometry(precision, variant, ngptot, nproma, klev, int(bool(laer)), C.byref(g)))
    return g.to_dict()


BATCH_MAX_SETS = 65535


def batch_launch_geometry(precision: int, nsets: int, ngptot: int, nproma: int, klev: int, laer: bool = False) -> dict:
    """What Batch.run would launch: launch_geometry of one set (KCACHE) with units and workgroups times nsets."""
    g = LaunchGeometry()
    check(gpu_lib().cloudsc_batch_launch_geometry(precision, nsets, ngptot, nproma, klev, int(bool(laer)), C.byref(g)))
    return g.to_dict()


class Batch:
    """cloudsc_batch_create / cloudsc_gpu_run_batch: `sets` (Fields of DEVICE pointers, or DeviceFields) of one
    shape run in ONE KCACHE launch, set i under params[i] (dicts keyed like Dataset.params) or, with params=None,
    all of them under the device's set (cloudsc_gpu_init).  Every selected output of set i has the bits
    gpu_run_outputs gives for that set alone under params[i].  Sets may share input members; the members the
    step writes (plude included) are exclusive.  The batch keeps its DeviceFields alive; the table and the
    parameter sets are uploaded once, here."""

    def __init__(self, sets, precision: int, outputs: int, ngptot: int, nproma: int, klev: int, params=None,
                 device: int = 0):
        self.lib = gpu_lib()
        self.h = None
        self.sets = list(sets)            # references: the device memory must outlive the batch
        self.device = device
        fs = [s.f if isinstance(s, DeviceFields) else s for s in self.sets]
        for f in fs:
            require_blocked(f, "Batch")
        if params is not None and len(params) != len(fs):
            raise ValueError("Batch: one parameter set per field set (%d sets, %d parameter sets)"
                             % (len(fs), len(params)))
        arr = (Fields * max(len(fs), 1))()
        for i, f in enumerate(fs):
            C.memmove(C.byref(arr, i * C.sizeof(Fields)), C.byref(f), C.sizeof(Fields))
        par = None
        if params is not None:
            par = (Params * max(len(fs), 1))()
            for i, d in enumerate(params):
                p = d if isinstance(d, Params) else Params.from_dict(d)
                C.memmove(C.byref(par, i * C.sizeof(Params)), C.byref(p), C.sizeof(Params))
        h = C.c_void_p()
        check(self.lib.cloudsc_batch_create(C.byref(h), device, precision, outputs, len(fs), ngptot, nproma, klev,
                                            arr, par))
        self.h = h

    @property
    def nsets(self) -> int:
        return self.lib.cloudsc_batch_nsets(self.h)

    def run(self, variant: int = None, stream=None) -> None:
        """One launch for every set, asynchronous on `stream` (None = the default stream); VARIANT_KCACHE only."""
        check(self.lib.cloudsc_gpu_run_batch(self.h, stream, VARIANT_KCACHE if variant is None else variant))

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.cloudsc_batch_destroy(self.h)
            self.h = None
        self.sets = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def kseg_spin_limit(limit: int = -1) -> None:
    """Diagnostic: polls before a KSEG consumer gives up (negative = default, 0 = fail at once)."""
    check(gpu_lib().cloudsc_debug_set_kseg_spin_limit(limit))


def cpu_run(ds: "Dataset", ngptot: int, nproma: int = 32, nthreads: int = 0, col_offset: int = 0,
            precision: int = FP64):
    """The library's CPU variant (cloudsc_cpu_run, BASELINE.json config 1) on a
    host block-layout state expanded from ds.  Returns (HostState, seconds).
    Explicitly a CPU run -- it is never used in place of a GPU run.
    precision: FP64, or MIXED (float arrays, double arithmetic)."""
    st = make_host_state(ds, ngptot, nproma, precision, col_offset)
    return st, cpu_run_state(ds, st, nthreads)


def cpu_run_state(ds: "Dataset", st: "HostState", nthreads: int = 0) -> float:
    """cloudsc_cpu_run_precision on an already expanded host state of precision
    FP64 or MIXED (plude is INOUT: the caller restores it between runs).
    Returns seconds of the block loop."""
    p = Params.from_dict(ds.params)
    f = st.fields()
    secs = C.c_double()
    check(gpu_lib().cloudsc_cpu_run_precision(nthreads, st.precision, st.ngptot, st.nproma, st.klev, C.byref(p),
                                              C.byref(f), C.byref(secs)))
    return secs.value


def fields_subset(f: "Fields", names=None, other: Optional["Fields"] = None) -> "Fields":
    """A Fields with only `names` copied from f (None: every member f holds -- and `other` holds, if given)."""
    out = Fields()
    for n in (ALL_FIELDS if names is None else names):
        if n not in ALL_FIELDS:
            raise KeyError("no such field: %s" % n)
        p = getattr(f, n)
        if names is None and (not p or (other is not None and not getattr(other, n))):
            continue
        setattr(out, n, p)
    return out


def convert_fields(src: "Fields", dst: "Fields", ngptot: int, klev: int, src_precision: int, src_nproma: int,
                   dst_precision: int, dst_nproma: int, device: int = 0, stream=None) -> None:
    """cloudsc_fields_convert: copy the members set in both DEVICE field sets into another NPROMA blocking
    and / or storage type, one kernel launch on `stream` (a hipStream_t value, None = the default stream).
    Asynchronous: synchronise the stream before reading dst from the host."""
    check(gpu_lib().cloudsc_fields_convert(device, stream, ngptot, klev, src_precision, src_nproma, C.byref(src),
                                           dst_precision, dst_nproma, C.byref(dst)))


def convert_fields_outputs(src: "Fields", dst: "Fields", ngptot: int, klev: int, outputs: int, src_precision: int,
                           src_nproma: int, dst_precision: int, dst_nproma: int, device: int = 0,
                           stream=None) -> None:
    """cloudsc_fields_convert_outputs: convert_fields for two sets of one output selection -- with
    OUTPUTS_SURFACE the SURFACE_FLUX_FIELDS members of both are surface fields."""
    check(gpu_lib().cloudsc_fields_convert_outputs(device, stream, ngptot, klev, outputs, src_precision, src_nproma,
                                                   C.byref(src), dst_precision, dst_nproma, C.byref(dst)))


def convert_fields_layout(src: "Fields", dst: "Fields", ngptot: int, klev: int, src_precision: int, src_layout: int,
                          src_nproma: int, dst_precision: int, dst_layout: int, dst_nproma: int,
                          outputs: int = OUTPUTS_ALL, device: int = 0, stream=None) -> None:
    """cloudsc_fields_convert_layout: convert_fields_outputs between DEVICE field sets of either layout
    (LAYOUT_BLOCKED: [nblocks][rows][nproma]; LAYOUT_LEVELS: [ngptot][rows], its nproma 0).  Asynchronous on
    `stream`: synchronise it before reading dst from the host."""
    check(gpu_lib().cloudsc_fields_convert_layout(device, stream, ngptot, klev, outputs, src_precision, src_layout,
                                                  src_nproma, C.byref(src), dst_precision, dst_layout, dst_nproma,
                                                  C.byref(dst)))


def cpu_convert_fields_layout(src: "Fields", dst: "Fields", ngptot: int, klev: int, src_precision: int,
                              src_layout: int, src_nproma: int, dst_precision: int, dst_layout: int, dst_nproma: int,
                              outputs: int = OUTPUTS_ALL, nthreads: int = 0) -> None:
    """cloudsc_cpu_fields_convert_layout: the same on two Fields of HOST pointers."""
    check(gpu_lib().cloudsc_cpu_fields_convert_layout(nthreads, ngptot, klev, outputs, src_precision, src_layout,
                                                      src_nproma, C.byref(src), dst_precision, dst_layout,
                                                      dst_nproma, C.byref(dst)))


def cpu_convert_fields(src, dst, ngptot: Optional[int] = None, klev: Optional[int] = None,
                       src_precision: Optional[int] = None, src_nproma: Optional[int] = None,
                       dst_precision: Optional[int] = None, dst_nproma: Optional[int] = None, names=None,
                       nthreads: int = 0) -> None:
    """cloudsc_cpu_fields_convert on host arrays.  src / dst: a HostState (its shape and precision are
    taken from it, and `names` -- default: the arrays both states hold -- selects the members) or a plain
    Fields of host pointers (every shape argument is then needed; names must be None)."""
    def unpack(x, precision, nproma):
        if isinstance(x, HostState):
            return x.fields(), x.ngptot, x.klev, x.precision, x.nproma
        if precision is None or nproma is None:
            raise ValueError("a plain Fields needs its precision and nproma")
        return x, ngptot, klev, precision, nproma
    sf, sn, sk, sp, snp = unpack(src, src_precision, src_nproma)
    df, dn, dk, dp, dnp = unpack(dst, dst_precision, dst_nproma)
    n, k = (sn if ngptot is None else ngptot), (sk if klev is None else klev)
    if n is None or k is None or dn not in (None, n) or dk not in (None, k):
        raise ValueError("ngptot / klev missing or not the same for src and dst")
    if isinstance(src, HostState) and isinstance(dst, HostState):
        sf, df = fields_subset(sf, names, df), fields_subset(df, names, sf)
    elif names is not None:
        raise ValueError("names needs two HostStates")
    check(gpu_lib().cloudsc_cpu_fields_convert(nthreads, n, k, sp, snp, C.byref(sf), dp, dnp, C.byref(df)))


# Packed tendency buffers (the reference's Fortran drivers' BUFFER_TMP / BUFFER_LOC, include/cloudsc_amd.h):
# [nblocks][tend_planes][klev][nproma], the reference's plane order T, A, Q, CLD(1..5)
TENDBUF_PLANES_MIN, TENDBUF_PLANES_MAX = 8, 64
TENDBUF_T, TENDBUF_A, TENDBUF_Q, TENDBUF_CLD = 0, 1, 2, 3
TENDENCY_FIELDS = tuple(n for n in ALL_FIELDS if n.startswith("tendency_"))


def bind_tendbuf(f: "Fields", precision: int, nproma: int, klev: int, buffer_tmp: int, buffer_loc: int) -> None:
    """cloudsc_tendbuf_bind: the eight tendency members of f = the plane starts of the two buffers (host or
    device addresses) in the reference's plane order."""
    check(gpu_lib().cloudsc_tendbuf_bind(C.byref(f), precision, nproma, klev, buffer_tmp, buffer_loc))


def gpu_run_tendbuf(f: "Fields", precision: int, variant: int, ngptot: int, nproma: int, klev: int,
                    tend_planes: int, scratch=None, device: int = 0, stream=None) -> None:
    """cloudsc_gpu_run_tendbuf: one step on DEVICE fields whose tendency members are planes of packed
    buffers of tend_planes planes per block.  Asynchronous on `stream`; KSEG callers follow it with
    cloudsc_gpu_check."""
    require_blocked(f, "gpu_run_tendbuf")
    check(gpu_lib().cloudsc_gpu_run_tendbuf(device, stream, precision, variant, ngptot, nproma, klev, tend_planes,
                                            C.byref(f), scratch))


def cpu_run_tendbuf(params: "Params", f: "Fields", precision: int, ngptot: int, nproma: int, klev: int,
                    tend_planes: int, nthreads: int = 0) -> None:
    """cloudsc_cpu_run_tendbuf: the CPU variant on HOST fields whose tendency members are planes of packed
    buffers (precision FP64 or MIXED)."""
    require_blocked(f, "cpu_run_tendbuf")
    check(gpu_lib().cloudsc_cpu_run_tendbuf(nthreads, precision, ngptot, nproma, klev, tend_planes, C.byref(params),
                                            C.byref(f)))


def gpu_run_outputs(f: "Fields", precision: int, variant: int, outputs: int, ngptot: int, nproma: int, klev: int,
                    scratch=None, device: int = 0, stream=None) -> None:
    """cloudsc_gpu_run_outputs: one step on DEVICE fields with an output selection.  OUTPUTS_ALL is
    cloudsc_gpu_run; with OUTPUTS_PROGNOSTIC the DIAGNOSTIC_FLUX_FIELDS members are neither read nor written
    (they may be None).  Asynchronous on `stream`; KSEG callers follow it with cloudsc_gpu_check."""
    require_blocked(f, "gpu_run_outputs")
    check(gpu_lib().cloudsc_gpu_run_outputs(device, stream, precision, variant, outputs, ngptot, nproma, klev,
                                            C.byref(f), scratch))


def cpu_run_outputs(params: "Params", f: "Fields", precision: int, outputs: int, ngptot: int, nproma: int,
                    klev: int, nthreads: int = 0) -> None:
    """cloudsc_cpu_run_outputs: the CPU variant on HOST fields with an output selection (precision FP64 or
    MIXED)."""
    require_blocked(f, "cpu_run_outputs")
    check(gpu_lib().cloudsc_cpu_run_outputs(nthreads, precision, outputs, ngptot, nproma, klev, C.byref(params),
                                            C.byref(f)))


def gpu_run_tendbuf_outputs(f: "Fields", precision: int, variant: int, outputs: int, ngptot: int, nproma: int,
                            klev: int, tend_planes: int, scratch=None, device: int = 0, stream=None) -> None:
    """cloudsc_gpu_run_tendbuf_outputs: gpu_run_tendbuf with an output selection.  OUTPUTS_ALL is
    cloudsc_gpu_run_tendbuf; with OUTPUTS_PROGNOSTIC the DIAGNOSTIC_FLUX_FIELDS members are neither read nor
    written (they may be None).  Asynchronous on `stream`; KSEG callers follow it with cloudsc_gpu_check."""
    require_blocked(f, "gpu_run_tendbuf_outputs")
    check(gpu_lib().cloudsc_gpu_run_tendbuf_outputs(device, stream, precision, variant, outputs, ngptot, nproma,
                                                    klev, tend_planes, C.byref(f), scratch))


def cpu_run_tendbuf_outputs(params: "Params", f: "Fields", precision: int, outputs: int, ngptot: int, nproma: int,
                            klev: int, tend_planes: int, nthreads: int = 0) -> None:
    """cloudsc_cpu_run_tendbuf_outputs: the CPU variant on HOST fields whose tendency members are planes of
    packed buffers, with an output selection (precision FP64 or MIXED)."""
    require_blocked(f, "cpu_run_tendbuf_outputs")
    check(gpu_lib().cloudsc_cpu_run_tendbuf_outputs(nthreads, precision, outputs, ngptot, nproma, klev, tend_planes,
                                                    C.byref(params), C.byref(f)))


def bind_tendbuf_cml(precision: int, nproma: int, klev: int, buffer_cml: int) -> "TendCml":
    """cloudsc_tendbuf_bind_cml: the four cumulative plane starts of a packed buffer (host or device address)
    in the reference's plane order."""
    cml = TendCml()
    check(gpu_lib().cloudsc_tendbuf_bind_cml(C.byref(cml), precision, nproma, klev, buffer_cml))
    return cml


def bind_tendbuf_three(f: "Fields", precision: int, nproma: int, klev: int, buffer_tmp: int, buffer_cml: int,
                       buffer_loc: Optional[int] = None) -> tuple:
    """The three buffers of a Fortran-driver caller bound in the reference's plane order: the tendency_tmp_*
    members of f to buffer_tmp, the returned TendCml to buffer_cml, and tendency_loc_* to buffer_loc -- or to
    None where the caller keeps no BUFFER_LOC (the fused form, gpu_run_tendbuf_cml, never touches them).
    Returns (f, cml)."""
    if buffer_loc is None:
        bind_tendbuf(f, precision, nproma, klev, buffer_tmp, buffer_tmp)
        for n in ("tendency_loc_t", "tendency_loc_q", "tendency_loc_a", "tendency_loc_cld"):
            setattr(f, n, None)
    else:
        bind_tendbuf(f, precision, nproma, klev, buffer_tmp, buffer_loc)
    return f, bind_tendbuf_cml(precision, nproma, klev, buffer_cml)


def gpu_run_tendbuf_cml(f: "Fields", cml: "TendCml", precision: int, variant: int, outputs: int, ngptot: int,
                        nproma: int, klev: int, tend_planes: int, scratch=None, device: int = 0, stream=None) -> None:
    """cloudsc_gpu_run_tendbuf_cml: the prognostic (or surface) step on packed tendency buffers with its seven
    local tendencies ADDED to the cumulative planes `cml` instead of stored to tendency_loc_* (which may be
    None and are never touched).  fp64 / fp32: cml += loc, one add in the storage type; mixed: cml =
    float32(float64(cml) + loc64).  The vapour plane of cml is neither read nor written.  OUTPUTS_ALL is
    refused.  A launch adds once: repeated launches accumulate repeatedly.  Asynchronous."""
    require_blocked(f, "gpu_run_tendbuf_cml")
    check(gpu_lib().cloudsc_gpu_run_tendbuf_cml(device, stream, precision, variant, outputs, ngptot, nproma, klev,
                                                tend_planes, C.byref(f), C.byref(cml), scratch))


def cpu_run_tendbuf_cml(params: "Params", f: "Fields", cml: "TendCml", precision: int, outputs: int, ngptot: int,
                        nproma: int, klev: int, tend_planes: int, nthreads: int = 0) -> None:
    """cloudsc_cpu_run_tendbuf_cml: the same on HOST memory (fp64 and mixed)."""
    require_blocked(f, "cpu_run_tendbuf_cml")
    check(gpu_lib().cloudsc_cpu_run_tendbuf_cml(nthreads, precision, outputs, ngptot, nproma, klev, tend_planes,
                                                C.byref(params), C.byref(f), C.byref(cml)))


def gpu_run_spp(f: "Fields", spp: "Spp", precision: int, variant: int, outputs: int, ngptot: int, nproma: int,
                klev: int, scratch=None, device: int = 0, stream=None) -> None:
    """cloudsc_gpu_run_spp: gpu_run_outputs (OUTPUTS_ALL or OUTPUTS_PROGNOSTIC) with per-column multipliers of
    RAMID, RCLDIFF, RCLCRIT_SEA/LAND, RLCRITSNOW and RPECONS: `spp` holds DEVICE surface fields [nblocks][nproma]
    in the storage type, or None where a parameter is not perturbed (at least one is set).  Each column
    has the bits of the ordinary step under its own host-scaled parameter set.  Asynchronous."""
    require_blocked(f, "gpu_run_spp")
    check(gpu_lib().cloudsc_gpu_run_spp(device, stream, precision, variant, outputs, ngptot, nproma, klev, C.byref(f),
                                        C.byref(spp), scratch))


def cpu_run_spp(params: "Params", f: "Fields", spp: "Spp", precision: int, outputs: int, ngptot: int, nproma: int,
                klev: int, nthreads: int = 0) -> None:
    """cloudsc_cpu_run_spp: the same on HOST memory (fp64 and mixed)."""
    require_blocked(f, "cpu_run_spp")
    check(gpu_lib().cloudsc_cpu_run_spp(nthreads, precision, outputs, ngptot, nproma, klev, C.byref(params),
                                        C.byref(f), C.byref(spp)))


def gpu_run_advance(f: "Fields", adv: "Advance", precision: int, variant: int, outputs: int, ngptot: int,
                    nproma: int, klev: int, scratch=None, device: int = 0, stream=None) -> None:
    """cloudsc_gpu_run_advance: the step (OUTPUTS_ALL or OUTPUTS_SURFACE) with the updated prognostics X_new =
    (X + ptsphy * tendency_tmp) + ptsphy * tendency_loc stored to `adv` instead of the seven local tendencies
    (tendency_loc_* may be None and are never touched).  Each member of adv is the set's own state member (in
    place: Advance.in_place(f)) or another DEVICE array.  Working type: double for fp64 and mixed (mixed =
    float32(fp64 form(float64 inputs))), float for fp32.  Asynchronous; N calls in place integrate N steps."""
    require_blocked(f, "gpu_run_advance")
    check(gpu_lib().cloudsc_gpu_run_advance(device, stream, precision, variant, outputs, ngptot, nproma, klev,
                                            C.byref(f), C.byref(adv), scratch))


def cpu_run_advance(params: "Params", f: "Fields", adv: "Advance", precision: int, outputs: int, ngptot: int,
                    nproma: int, klev: int, nthreads: int = 0) -> None:
    """cloudsc_cpu_run_advance: the same on HOST memory (fp64 and mixed)."""
    require_blocked(f, "cpu_run_advance")
    check(gpu_lib().cloudsc_cpu_run_advance(nthreads, precision, outputs, ngptot, nproma, klev, C.byref(params),
                                            C.byref(f), C.byref(adv)))


def advance_fields(f: "Fields", adv: "Advance", precision: int, ngptot: int, nproma: int, klev: int,
                   device: int = 0, stream=None) -> None:
    """cloudsc_fields_advance: the separate pass on the device over a set whose tendency_loc_* a step has filled,
    with ptsphy of the device's parameter set.  Equal to the fused form bit for bit in fp64 and fp32; in mixed
    it can only take the stored (narrowed) tendency, so some elements differ in the last bit.  Asynchronous."""
    require_blocked(f, "advance_fields")
    check(gpu_lib().cloudsc_fields_advance(device, stream, precision, ngptot, nproma, klev, C.byref(f), C.byref(adv)))


def cpu_advance_fields(params: "Params", f: "Fields", adv: "Advance", precision: int, ngptot: int, nproma: int,
                       klev: int, nthreads: int = 0) -> None:
    """cloudsc_cpu_fields_advance: the same on HOST arrays with ptsphy from `params` (all three precisions)."""
    require_blocked(f, "cpu_advance_fields")
    check(gpu_lib().cloudsc_cpu_fields_advance(nthreads, precision, ngptot, nproma, klev, C.byref(params), C.byref(f),
                                               C.byref(adv)))


def accumulate_tendbuf(loc: "Fields", cml: "TendCml", precision: int, ngptot: int, nproma: int, klev: int,
                       loc_tend_planes: int, cml_tend_planes: int, device: int = 0, stream=None) -> None:
    """cloudsc_fields_accumulate_tendbuf: cml += tendency_loc_* of `loc` over the seven planes on the device,
    one add in the storage type (float for fp32 and mixed: the stored float is added, unlike the fused form's
    mixed rule).  *_tend_planes: 0 for separate arrays, 8..64 for planes of a packed buffer.  Asynchronous."""
    check(gpu_lib().cloudsc_fields_accumulate_tendbuf(device, stream, precision, ngptot, nproma, klev,
                                                      loc_tend_planes, C.byref(loc), cml_tend_planes, C.byref(cml)))


def cpu_accumulate_tendbuf(loc: "Fields", cml: "TendCml", precision: int, ngptot: int, nproma: int, klev: int,
                           loc_tend_planes: int, cml_tend_planes: int, nthreads: int = 0) -> None:
    """cloudsc_cpu_fields_accumulate_tendbuf: the same on HOST arrays."""
    check(gpu_lib().cloudsc_cpu_fields_accumulate_tendbuf(nthreads, precision, ngptot, nproma, klev, loc_tend_planes,
                                                          C.byref(loc), cml_tend_planes, C.byref(cml)))


def convert_fields_tendbuf(src: "Fields", dst: "Fields", ngptot: int, klev: int, src_precision: int,
                           src_nproma: int, src_tend_planes: int, dst_precision: int, dst_nproma: int,
                           dst_tend_planes: int, device: int = 0, stream=None) -> None:
    """cloudsc_fields_convert_tendbuf: convert_fields with the tendency members of src and / or dst in packed
    buffers (*_tend_planes planes per block, 0 = separate arrays): pack, unpack or re-pack in one launch."""
    check(gpu_lib().cloudsc_fields_convert_tendbuf(device, stream, ngptot, klev, src_precision, src_nproma,
                                                   src_tend_planes, C.byref(src), dst_precision, dst_nproma,
                                                   dst_tend_planes, C.byref(dst)))


def cpu_convert_fields_tendbuf(src: "Fields", dst: "Fields", ngptot: int, klev: int, src_precision: int,
                               src_nproma: int, src_tend_planes: int, dst_precision: int, dst_nproma: int,
                               dst_tend_planes: int, nthreads: int = 0) -> None:
    """cloudsc_cpu_fields_convert_tendbuf: the same on HOST arrays."""
    check(gpu_lib().cloudsc_cpu_fields_convert_tendbuf(nthreads, ngptot, klev, src_precision, src_nproma,
                                                       src_tend_planes, C.byref(src), dst_precision, dst_nproma,
                                                       dst_tend_planes, C.byref(dst)))


def _diffs_to_dict(diffs) -> Dict[str, dict]:
    return {n: d.to_dict() for n, d in zip(ALL_FIELDS, diffs) if d.compared}


def compare_fields(a: "Fields", b: "Fields", ngptot: int, klev: int, a_precision: int, a_nproma: int,
                   b_precision: int, b_nproma: int, device: int = 0, stream=None) -> Dict[str, dict]:
    """cloudsc_fields_compare: the members set in both DEVICE field sets, a against b as the reference, in
    one streaming pass on `stream` (waits for that stream).  {member: {"stats": the 7-tuple of
    GpuState.validate, "compared", "mismatches" (elements that differ as bits), "first": (global column,
    row) of the first mismatch or None}} for the members compared."""
    diffs = (FieldDiff * len(ALL_FIELDS))()
    check(gpu_lib().cloudsc_fields_compare(device, stream, ngptot, klev, a_precision, a_nproma, C.byref(a),
                                           b_precision, b_nproma, C.byref(b), diffs))
    return _diffs_to_dict(diffs)


def compare_fields_outputs(a: "Fields", b: "Fields", ngptot: int, klev: int, outputs: int, a_precision: int,
                           a_nproma: int, b_precision: int, b_nproma: int, device: int = 0,
                           stream=None) -> Dict[str, dict]:
    """cloudsc_fields_compare_outputs: compare_fields for two sets of one output selection -- with
    OUTPUTS_SURFACE the SURFACE_FLUX_FIELDS members of both are surface fields (one row)."""
    diffs = (FieldDiff * len(ALL_FIELDS))()
    check(gpu_lib().cloudsc_fields_compare_outputs(device, stream, ngptot, klev, outputs, a_precision, a_nproma,
                                                   C.byref(a), b_precision, b_nproma, C.byref(b), diffs))
    return _diffs_to_dict(diffs)


def cpu_compare_fields(a: "HostState", b: "HostState", names=None, nthreads: int = 0) -> Dict[str, dict]:
    """cloudsc_cpu_fields_compare on two HostStates of the same ngptot and klev (any two blockings and
    precisions): the members in `names`, or every array both hold.  Same result shape as compare_fields."""
    if (a.ngptot, a.klev) != (b.ngptot, b.klev):
        raise ValueError("cpu_compare_fields: ngptot and klev must be the same")
    fa, fb = a.fields(), b.fields()
    fa, fb = fields_subset(fa, names, fb), fields_subset(fb, names, fa)
    diffs = (FieldDiff * len(ALL_FIELDS))()
    check(gpu_lib().cloudsc_cpu_fields_compare(nthreads, a.ngptot, a.klev, a.precision, a.nproma, C.byref(fa),
                                               b.precision, b.nproma, C.byref(fb), diffs))
    return _diffs_to_dict(diffs)


def compare_fields_tendbuf(a: "Fields", b: "Fields", ngptot: int, klev: int, a_precision: int, a_nproma: int,
                           a_tend_planes: int, b_precision: int, b_nproma: int, b_tend_planes: int,
                           device: int = 0, stream=None) -> Dict[str, dict]:
    """cloudsc_fields_compare_tendbuf: compare_fields with the tendency members of a and / or b read in place
    from packed buffers (*_tend_planes planes per block, 0 = separate arrays)."""
    diffs = (FieldDiff * len(ALL_FIELDS))()
    check(gpu_lib().cloudsc_fields_compare_tendbuf(device, stream, ngptot, klev, a_precision, a_nproma,
                                                   a_tend_planes, C.byref(a), b_precision, b_nproma, b_tend_planes,
                                                   C.byref(b), diffs))
    return _diffs_to_dict(diffs)


def cpu_compare_fields_tendbuf(a: "Fields", b: "Fields", ngptot: int, klev: int, a_precision: int, a_nproma: int,
                               a_tend_planes: int, b_precision: int, b_nproma: int, b_tend_planes: int,
                               nthreads: int = 0) -> Dict[str, dict]:
    """cloudsc_cpu_fields_compare_tendbuf: the same on HOST arrays."""
    diffs = (FieldDiff * len(ALL_FIELDS))()
    check(gpu_lib().cloudsc_cpu_fields_compare_tendbuf(nthreads, ngptot, klev, a_precision, a_nproma, a_tend_planes,
                                                       C.byref(a), b_precision, b_nproma, b_tend_planes, C.byref(b),
                                                       diffs))
    return _diffs_to_dict(diffs)


def validate_fields_tendbuf(f: "Fields", ref: "Reference", precision: int, ngptot: int, nproma: int, klev: int,
                            tend_planes: int, outputs: int = OUTPUTS_ALL, col_offset: int = 0, device: int = 0,
                            stream=None) -> list:
    """cloudsc_fields_validate_tendbuf: the validated members of DEVICE fields against the KLON-column
    reference, the tendency members read in place from packed buffers (tend_planes 0 = separate arrays).  With
    OUTPUTS_PROGNOSTIC the DIAGNOSTIC_FLUX_FIELDS members and their reference arrays may be None: their
    records are the skipped record; with OUTPUTS_SURFACE the SURFACE_FLUX_FIELDS members are surface fields
    held against row klev of their reference profiles.  Returns the Stats array in VALIDATED order (waits for `stream`)."""
    stats = (Stats * len(VALIDATED))()
    check(gpu_lib().cloudsc_fields_validate_tendbuf(device, stream, precision, ngptot, nproma, klev, tend_planes,
                                                    outputs, col_offset, C.byref(f), C.byref(ref), stats))
    return stats


def expand_fields_tendbuf(f: "Fields", tmpl: "Template", precision: int, ngptot: int, nproma: int, tend_planes: int,
                          col_offset: int = 0, device: int = 0, stream=None) -> None:
    """cloudsc_fields_expand_tendbuf: fill the non-None input members of DEVICE fields from the template,
    tendency_tmp_* straight into their planes of a packed buffer.  Asynchronous on `stream`."""
    check(gpu_lib().cloudsc_fields_expand_tendbuf(device, stream, precision, ngptot, nproma, tend_planes, col_offset,
                                                  C.byref(tmpl), C.byref(f)))


def compare_grid(workgroups: int = 0) -> None:
    """Diagnostic: workgroups of the comparison kernel (0 = default); only the sums' low parts may change."""
    check(gpu_lib().cloudsc_debug_set_compare_grid(workgroups))


def validate_host_state(ds: "Dataset", st: "HostState") -> float:
    """Worst per-field relative L1 error (ERROR_PRINT, validate_mod.F90:263-296)
    of a host state's 21 outputs against ds.reference replicated with g % klon."""
    worst = 0.0
    io = io_lib()
    cols = None
    for _, k in VALIDATED:
        if io is not None:
            ref = np.ascontiguousarray(ds.reference[k], dtype=np.float64)
            fld = np.ascontiguousarray(st.arrays[k])
            stt = Stats()
            io.cloudsc_io_field_stats(ref.ctypes.data, _KIND_CODE[ALL_FIELDS[k]], ds.klev, ds.klon, fld.ctypes.data,
                                      fld.itemsize, st.ngptot, st.nproma, 0, C.byref(stt))
            errsum, refsum = stt.errsum, stt.refsum
        else:
            cols = np.arange(st.ngptot) % ds.klon if cols is None else cols
            out = blocks_to_columns(st.arrays[k], st.ngptot)
            _, _, _, errsum, refsum = field_stats(out, np.take(ds.reference[k], cols, axis=-1))
        worst = max(worst, rel_error(errsum, refsum)[0])
    return worst


# the translation unit of the CLOUDSC kernels (cloudsc_gpu.hip and what it includes)
KERNEL_SOURCES = ("cloudsc_gpu.hip", "cloudsc_kcache.h", "cloudsc_physics_level.inc", "cloudsc_scc.h", "cloudsc_dev.h",
                  "cloudsc_params.h", "cloudsc_libm.h", "cloudsc_libm_tab.h", "cloudsc_internal.h", "cloudsc_fields.def")


def kernel_source_hash() -> str:
    """SHA-256 (16 hex digits) of the kernels' sources and the library's build
    flags (Makefile): the key that ties a measured PMC traffic figure to the
    kernel it was measured on (bench.py drops a figure whose hash is not the
    current one)."""
    import hashlib
    h = hashlib.sha256()
    for name in KERNEL_SOURCES + ("../../include/cloudsc_amd.h", "../Makefile"):
        h.update(name.encode())
        with open(os.path.normpath(os.path.join(HERE, "csrc", name)), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def hbm_copy_gbps(device: int = 0, nbytes: int = 4 << 30, reps: int = 10) -> float:
    """Achievable HBM bandwidth of the device (STREAM copy, GB/s)."""
    g = C.c_double()
    check(gpu_lib().cloudsc_hbm_copy_gbps(device, nbytes, reps, C.byref(g)))
    return g.value


def pcie_gbps(device: int = 0, nbytes: int = 1 << 30, reps: int = 3) -> Dict[str, float]:
    """Host<->device copy ceiling (cloudsc_pcie_gbps): GB/s of H2D alone, D2H
    alone, and the total of both directions at once."""
    h, d, b = C.c_double(), C.c_double(), C.c_double()
    check(gpu_lib().cloudsc_pcie_gbps(device, nbytes, reps, C.byref(h), C.byref(d), C.byref(b)))
    return {"h2d": h.value, "d2h": d.value, "both": b.value}


def device_count() -> int:
    """Visible HIP devices (through the library; raises if it is missing)."""
    n = C.c_int(0)
    check(gpu_lib().cloudsc_gpu_device_count(C.byref(n)))
    return n.value


def check(rc: int) -> None:
    if rc != 0:
        lib = gpu_lib()
        raise CloudscError("cloudsc error %d: %s (hip: %s)" % (
            rc, lib.cloudsc_strerror(rc).decode(), (lib.cloudsc_last_hip_error() or b"").decode()), rc)


def make_template(ds: Dataset, keep: list) -> Template:
    t = Template()
    t.klon, t.klev = ds.klon, ds.klev
    for name, _ in Template._fields_[2:]:
        a = ds.inputs.get(name)
        if a is not None:
            a = np.ascontiguousarray(a)
            keep.append(a)
            setattr(t, name, a.ctypes.data)
    return t


def make_reference(ds: Dataset, keep: list) -> Reference:
    r = Reference()
    r.klon, r.klev = ds.klon, ds.klev
    for i, (_, key) in enumerate(VALIDATED):
        a = np.ascontiguousarray(ds.reference[key], dtype=np.float64)
        keep.append(a)
        r.field[i] = a.ctypes.data
    return r


class GpuState:
    """Device-resident CLOUDSC problem (cloudsc_state_* of cloudsc_amd.h)."""

    def __init__(self, ds: Dataset, ngptot: int, nproma: int = 128, precision: int = FP64,
                 device: int = 0, col_offset: int = 0):
        self.lib = gpu_lib()
        self.ds, self.ngptot, self.nproma, self.precision = ds, ngptot, nproma, precision
        keep: list = []
        tmpl = make_template(ds, keep)
        self._params = Params.from_dict(ds.params)
        h = C.c_void_p()
        check(self.lib.cloudsc_state_create(C.byref(h), device, precision, ngptot, nproma,
                                            col_offset, C.byref(tmpl), C.byref(self._params)))
        self.h = h

    def run(self, variant: int = VARIANT_KCACHE, reps: int = 1) -> np.ndarray:
        ms = (C.c_float * reps)()
        check(self.lib.cloudsc_state_run(self.h, variant, reps, ms))
        return np.array(ms[:], dtype=np.float64)

    def run_span(self, variant: int = VARIANT_KCACHE, reps: int = 1) -> float:
        """`reps` plain launches timed as a whole (cloudsc_state_run_span): ms from
        the first launch's start to the last one's end."""
        ms = C.c_float()
        check(self.lib.cloudsc_state_run_span(self.h, variant, reps, C.byref(ms)))
        return float(ms.value)

    def sync(self) -> None:
        check(self.lib.cloudsc_state_sync(self.h))

    def kseg_clock(self, reset: bool = False) -> float:
        """Effective shader clock (GHz) of the KSEG launches since the last reset
        (cloudsc_state_kseg_clock); 0.0 before any KSEG launch."""
        ghz = C.c_double()
        check(self.lib.cloudsc_state_kseg_clock(self.h, int(reset), C.byref(ghz)))
        return ghz.value

    def placement(self) -> dict:
        """The output placement search of this state (cloudsc_state_placement)."""
        a, b, t, m = C.c_float(), C.c_float(), C.c_int(), C.c_int()
        check(self.lib.cloudsc_state_placement(self.h, C.byref(a), C.byref(b), C.byref(t), C.byref(m)))
        return {"probe_first_ms": round(a.value, 4), "probe_final_ms": round(b.value, 4),
                "tries": t.value, "moves": m.value}

    def placement_report(self) -> dict:
        """The placement search with its cost (cloudsc_state_placement_report)."""
        r = Placement()
        check(self.lib.cloudsc_state_placement_report(self.h, C.byref(r)))
        return r.to_dict()

    def reset(self) -> None:
        check(self.lib.cloudsc_state_reset(self.h))

    def validate(self, ds: Optional[Dataset] = None) -> list:
        ds = ds or self.ds
        keep: list = []
        ref = make_reference(ds, keep)
        st = (Stats * 21)()
        check(self.lib.cloudsc_state_validate(self.h, C.byref(ref), st))
        # (min, max, max|d|, sum|d|, sum|ref|, and the low parts of the two
        # double-double sums: cloudsc_dist.combine_stats adds partials exactly)
        return [(s.minval, s.maxval, s.maxerr, s.errsum, s.refsum, s.errsum_lo, s.refsum_lo) for s in st]

    def download(self, key: str) -> np.ndarray:
        idx = [k for _, k in VALIDATED].index(key)
        n = self.lib.cloudsc_state_field_elems(self.h, idx)
        out = np.empty(n, dtype=np.float64)
        check(self.lib.cloudsc_state_download(self.h, idx, out.ctypes.data))
        nb = nblocks_of(self.ngptot, self.nproma)
        return out.reshape((nb,) + field_shape(ALL_FIELDS[key], self.ds.klev, self.nproma))

    def outputs(self) -> Dict[str, np.ndarray]:
        """All 21 validated fields, column-last template-like order [..][ngptot]."""
        return {k: blocks_to_columns(self.download(k), self.ngptot) for _, k in VALIDATED}

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.cloudsc_state_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostPipeline:
    """Host-buffer CLOUDSC step (cloudsc_host_pipeline_* of cloudsc_amd.h): the
    block-layout arrays live in host memory (pinned in place) and every step
    copies inputs in and outputs out, chunked and overlapped over streams."""

    def __init__(self, ds: Dataset, ngptot: int, nproma: int = 128, precision: int = FP64, device: int = 0,
                 chunk_blocks: int = 128, nstreams: int = 3, col_offset: int = 0, packed: bool = False):
        """packed: all arrays carved back to back (8-byte gaps) out of ONE host
        buffer, so that neighbouring fields share pages -- the layout that
        exercises the pipeline's page-merged pinning."""
        self.lib = gpu_lib()
        self.ds, self.ngptot, self.nproma, self.precision = ds, ngptot, nproma, precision
        self._params = Params.from_dict(ds.params)
        check(self.lib.cloudsc_gpu_init(device, C.byref(self._params)))
        self.state = make_host_state(ds, ngptot, nproma, precision, col_offset)
        if packed:
            arrs = self.state.arrays
            self._buf = np.empty(sum(a.nbytes + 8 for a in arrs.values()) + 64, dtype=np.uint8)
            off = 8 - self._buf.ctypes.data % 8
            for name, a in list(arrs.items()):
                v = self._buf[off:off + a.nbytes].view(a.dtype).reshape(a.shape)
                v[...] = a
                arrs[name] = v
                off += a.nbytes + 8
        self._plude0 = self.state.arrays["plude"].copy()
        f = self.state.fields()
        if not (ds.params.get("laericesed") or ds.params.get("laericeauto")):
            for name in AEROSOL_FIELDS:            # not read by the kernel: not transferred
                setattr(f, name, None)
        self._fields = f
        h = C.c_void_p()
        check(self.lib.cloudsc_host_pipeline_create(C.byref(h), device, precision, ngptot, nproma, ds.klev,
                                                    chunk_blocks, nstreams, C.byref(f)))
        self.h = h

    def run(self, variant: int = VARIANT_KCACHE) -> float:
        """One step; plude is restored on the host first (INOUT).  Returns ms."""
        np.copyto(self.state.arrays["plude"], self._plude0)
        ms = C.c_double()
        check(self.lib.cloudsc_host_pipeline_run(self.h, variant, C.byref(ms)))
        return ms.value

    def outputs(self) -> Dict[str, np.ndarray]:
        return state_outputs_to_template(self.state.arrays, self.ngptot)

    def mapping(self):
        """(arrays, arrays NOT covered by one pinned mapping) -- the pinning
        invariant of cloudsc_host_pipeline_create (cloudsc_debug_host_pipeline_mapping)."""
        n, bad = C.c_int(), C.c_int()
        check(self.lib.cloudsc_debug_host_pipeline_mapping(self.h, C.byref(n), C.byref(bad)))
        return n.value, bad.value

    def copy_path(self):
        """(mode, H2D engine mask, D2H engine mask) of this pipeline
        (cloudsc_debug_host_pipeline_copy): mode 1 = copy engines per direction,
        0 = HIP streams."""
        m, a, b = C.c_int(), C.c_int(), C.c_int()
        check(self.lib.cloudsc_debug_host_pipeline_copy(self.h, C.byref(m), C.byref(a), C.byref(b)))
        return m.value, a.value, b.value

    def copy_bound(self) -> float:
        """ms of one step's copies without the kernels, same engines and
        arrays (cloudsc_host_pipeline_copy_bound); clobbers the host outputs
        and plude (restored by the next run())."""
        t = C.c_double()
        check(self.lib.cloudsc_host_pipeline_copy_bound(self.h, C.byref(t)))
        return t.value

    def engine_check(self):
        """(overlap, pairs tried) of the engine pair check at creation
        (cloudsc_debug_host_pipeline_engine_check): overlap = both directions at
        once / the slower alone for the kept pair (1.0 = fully concurrent)."""
        o, n = C.c_double(), C.c_int()
        check(self.lib.cloudsc_debug_host_pipeline_engine_check(self.h, C.byref(o), C.byref(n)))
        return o.value, n.value

    def host_arrays(self):
        """(pointer, bytes) of every host array handed to the pipeline."""
        out = []
        for name, _ in Fields._fields_:
            p = getattr(self._fields, name)
            if p:
                out.append((p, self.state.arrays[name].nbytes))
        return out

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.cloudsc_host_pipeline_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _hip():
    h = C.CDLL("libamdhip64.so")
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipDeviceSynchronize.argtypes = []
    h.hipSetDevice.argtypes = [C.c_int]
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipFree.argtypes = [C.c_void_p]
    return h


class DeviceFields:
    """Caller-owned device fields (cloudsc_fields_alloc / cloudsc_fields_free):
    the reference CUDA driver's shape -- allocate (cloudsc_driver.cu:276-328),
    copy the inputs in, launch cloudsc_gpu_run (:391-416), copy the outputs
    back (:425-447) -- with the output buffers placed by the library's
    memory-pattern search (reads + writes, no physics) unless place=False.
    tend_planes (8..64): also allocate two packed tendency buffers of that many planes per block
    (self.buffer_tmp, self.buffer_loc, plain hipMalloc) and bind the eight tendency members of self.f to
    them in the reference's plane order -- the set then runs with gpu_run_tendbuf; self.separate keeps the
    set with the tendency members as the separate arrays cloudsc_fields_alloc made.
    outputs=OUTPUTS_PROGNOSTIC: cloudsc_fields_alloc_outputs -- the DIAGNOSTIC_FLUX_FIELDS members stay None and
    the placement search runs over the eleven other outputs; the set runs with gpu_run_outputs.
    outputs=OUTPUTS_SURFACE: likewise, and the SURFACE_FLUX_FIELDS members are surface fields [nblocks][nproma]
    (selected_field_shape): upload, download, copy_from, convert_to and compare take them as such, between
    sets of the same selection.
    layout=LAYOUT_LEVELS: the caller's level-contiguous arrays -- member `name` is (ngptot, rows) or (ngptot,)
    (shape), nproma must be 0, no placement search is done and tend_planes is refused.  upload, download and
    convert_to (cloudsc_fields_convert_layout when the two layouts differ) take such a set; the step wrappers,
    compare, validate and expand refuse it (self.f is a LevelsFields)."""

    def __init__(self, ngptot: int, nproma: int, klev: int, precision: int = FP64, device: int = 0,
                 place: bool = True, aerosols: bool = False, tend_planes: int = 0, outputs: int = OUTPUTS_ALL,
                 layout: int = LAYOUT_BLOCKED):
        if layout not in (LAYOUT_BLOCKED, LAYOUT_LEVELS):
            raise ValueError("unknown layout: %r" % (layout,))
        if layout == LAYOUT_LEVELS and (nproma or tend_planes):
            raise ValueError("a LAYOUT_LEVELS set has no NPROMA (pass 0) and no packed tendency buffers")
        self.lib = gpu_lib()
        self.ngptot, self.nproma, self.klev, self.precision, self.device = ngptot, nproma, klev, precision, device
        self.layout = layout
        self.f = Fields() if layout == LAYOUT_BLOCKED else LevelsFields()
        self.report = Placement()
        flags = (0 if place else PLACE_NONE) | (ALLOC_AEROSOLS if aerosols else 0)
        self.outputs = outputs
        if layout == LAYOUT_LEVELS:   # [ngptot][rows] has the elements of one block of ngptot columns: no padding
            nproma, flags = ngptot, flags | PLACE_NONE
        if outputs == OUTPUTS_ALL:
            check(self.lib.cloudsc_fields_alloc(device, precision, ngptot, nproma, klev, flags, C.byref(self.f),
                                                C.byref(self.report)))
        else:
            check(self.lib.cloudsc_fields_alloc_outputs(device, precision, ngptot, nproma, klev, flags, outputs,
                                                        C.byref(self.f), C.byref(self.report)))
        self.hip = _hip()
        self.tend_planes, self.separate, self.buffer_tmp, self.buffer_loc = 0, None, None, None
        if tend_planes:
            if not TENDBUF_PLANES_MIN <= tend_planes <= TENDBUF_PLANES_MAX:
                self.close()
                raise ValueError("tend_planes must be in %d..%d" % (TENDBUF_PLANES_MIN, TENDBUF_PLANES_MAX))
            self.separate = Fields()
            C.memmove(C.byref(self.separate), C.byref(self.f), C.sizeof(Fields))
            self.tend_planes = tend_planes
            self.hip.hipSetDevice(device)
            bufs = []
            for _ in range(2):
                p = C.c_void_p()
                if self.hip.hipMalloc(C.byref(p), self.tendbuf_nbytes()) != 0 or not p.value:
                    for q in bufs:
                        self.hip.hipFree(q)
                    self.tend_planes = 0
                    self.close()
                    raise CloudscError("hipMalloc of a tendency buffer failed")
                bufs.append(p.value)
            self.buffer_tmp, self.buffer_loc = bufs
            bind_tendbuf(self.f, precision, nproma, klev, self.buffer_tmp, self.buffer_loc)

    def tendbuf_nbytes(self) -> int:
        """Bytes of one packed tendency buffer of this set."""
        return (nblocks_of(self.ngptot, self.nproma) * self.tend_planes * self.klev * self.nproma *
                np.dtype(storage_dtype(self.precision)).itemsize)

    def nbytes(self, name: str) -> int:
        es = 4 if name == "ktype" else np.dtype(storage_dtype(self.precision)).itemsize
        if self._layout() == LAYOUT_LEVELS:
            return int(np.prod(self.shape(name))) * es
        return nblocks_of(self.ngptot, self.nproma) * int(np.prod(self.shape(name))) * es

    def shape(self, name: str) -> tuple:
        """The per-block shape of a member of this set (selected_field_shape of its output selection); of a
        LAYOUT_LEVELS set the whole member's: (ngptot, rows), or (ngptot,) for a member of one row."""
        per_column = selected_field_shape(name, self.klev, 1, self._selection())
        if self._layout() == LAYOUT_LEVELS:
            rows = int(np.prod(per_column))
            return (self.ngptot, rows) if len(per_column) > 1 else (self.ngptot,)
        return selected_field_shape(name, self.klev, self.nproma, self._selection())

    def _layout(self) -> int:
        return getattr(self, "layout", LAYOUT_BLOCKED)

    def _selection(self) -> int:
        """This set's output selection (OUTPUTS_ALL for a set put together without one)."""
        return getattr(self, "outputs", OUTPUTS_ALL)

    def _same_selection(self, other: "DeviceFields", what: str) -> None:
        if (self._selection() == OUTPUTS_SURFACE) != (other._selection() == OUTPUTS_SURFACE):
            raise ValueError("%s: one set holds the surface fluxes as surface fields, the other as profiles "
                             "(pass names without SURFACE_FLUX_FIELDS)" % what)

    def copy_from(self, src: "Fields", names) -> None:
        """Device-to-device copy of the named fields from another field set of
        the same configuration (e.g. a state's, cloudsc_state_fields)."""
        self.hip.hipSetDevice(self.device)
        for n in names:
            rc = self.hip.hipMemcpy(getattr(self.f, n), getattr(src, n), self.nbytes(n), 3)
            if rc != 0:
                raise CloudscError("hipMemcpy %s failed (%d)" % (n, rc))

    def upload(self, arrays: Dict[str, np.ndarray]) -> None:
        """Host arrays in this set's layout (block layout: make_host_state(...).arrays; LAYOUT_LEVELS:
        shape(name) each) into the device buffers."""
        self.hip.hipSetDevice(self.device)
        for n, a in arrays.items():
            if getattr(self.f, n, None) is None:
                continue
            a = np.ascontiguousarray(a)
            assert a.nbytes == self.nbytes(n), (n, a.nbytes, self.nbytes(n))
            rc = self.hip.hipMemcpy(getattr(self.f, n), a.ctypes.data, a.nbytes, 1)
            if rc != 0:
                raise CloudscError("hipMemcpy %s failed (%d)" % (n, rc))

    def convert_to(self, other: "DeviceFields", names=None, stream=None) -> None:
        """cloudsc_fields_convert of this set into `other` (another blocking and / or precision of the
        same ngptot and klev, same device): the members in `names`, or every member both sets hold.
        Asynchronous on `stream` (None = the default stream)."""
        if (other.ngptot, other.klev, other.device) != (self.ngptot, self.klev, self.device):
            raise ValueError("convert_to: ngptot, klev and device must be the same")
        a, b = fields_subset(self.f, names, other.f), fields_subset(other.f, names, self.f)
        surface = (OUTPUTS_SURFACE in (self._selection(), other._selection())
                   and any(getattr(a, n) for n in SURFACE_FLUX_FIELDS))
        if self._layout() != other._layout():
            if surface:
                self._same_selection(other, "convert_to")
            convert_fields_layout(a, b, self.ngptot, self.klev, self.precision, self._layout(), self.nproma,
                                  other.precision, other._layout(), other.nproma,
                                  OUTPUTS_SURFACE if surface else OUTPUTS_ALL, self.device, stream)
            return
        # (two LEVELS sets: one block of ngptot columns each, the same element positions)
        snp, dnp = (self.nproma or self.ngptot), (other.nproma or other.ngptot)
        if surface:
            self._same_selection(other, "convert_to")
            convert_fields_outputs(a, b, self.ngptot, self.klev, OUTPUTS_SURFACE, self.precision, snp,
                                   other.precision, dnp, self.device, stream)
            return
        convert_fields(a, b, self.ngptot, self.klev, self.precision, snp, other.precision, dnp, self.device, stream)

    def compare(self, other: "DeviceFields", names=None, stream=None) -> Dict[str, dict]:
        """cloudsc_fields_compare of this set against `other` as the reference (another blocking and / or
        precision of the same ngptot and klev, same device): the members in `names`, or every member both
        sets hold.  See compare_fields for the result."""
        if (other.ngptot, other.klev, other.device) != (self.ngptot, self.klev, self.device):
            raise ValueError("compare: ngptot, klev and device must be the same")
        require_blocked(self.f, "compare")
        require_blocked(other.f, "compare")
        a, b = fields_subset(self.f, names, other.f), fields_subset(other.f, names, self.f)
        if OUTPUTS_SURFACE in (self._selection(), other._selection()) and any(getattr(a, n) for n in SURFACE_FLUX_FIELDS):
            self._same_selection(other, "compare")
            return compare_fields_outputs(a, b, self.ngptot, self.klev, OUTPUTS_SURFACE, self.precision, self.nproma,
                                          other.precision, other.nproma, self.device, stream)
        return compare_fields(a, b, self.ngptot, self.klev, self.precision, self.nproma, other.precision,
                              other.nproma, self.device, stream)

    def validate(self, ds: "Dataset", col_offset: int = 0, stream=None) -> list:
        """cloudsc_fields_validate: the 21 validated fields against ds.reference on the device; the list
        of 7-tuples GpuState.validate returns.  (A tend_planes set: its separate arrays, self.separate --
        unpack BUFFER_LOC first, or validate it in place with validate_fields_tendbuf.)"""
        require_blocked(self.f, "validate")
        keep: list = []
        ref = make_reference(ds, keep)
        st = (Stats * 21)()
        check(self.lib.cloudsc_fields_validate(self.device, stream, self.precision, self.ngptot, self.nproma,
                                               self.klev, col_offset, C.byref(self.separate or self.f),
                                               C.byref(ref), st))
        return [(s.minval, s.maxval, s.maxerr, s.errsum, s.refsum, s.errsum_lo, s.refsum_lo) for s in st]

    def expand(self, ds: "Dataset", col_offset: int = 0, stream=None) -> None:
        """cloudsc_fields_expand: fill every input member this set holds (plude included) from the
        dataset's template on the device.  Asynchronous on `stream` (None = the default stream).
        (A tend_planes set: its separate arrays, self.separate -- pack tendency_tmp_* afterwards, or fill the buffers
        in place with expand_fields_tendbuf.)"""
        require_blocked(self.f, "expand")
        if ds.klev != self.klev:
            raise ValueError("expand: the dataset's klev is not this set's")
        keep: list = []
        tmpl = make_template(ds, keep)
        check(self.lib.cloudsc_fields_expand(self.device, stream, self.precision, self.ngptot, self.nproma,
                                             col_offset, C.byref(tmpl), C.byref(self.separate or self.f)))

    def download_raw(self, name: str) -> np.ndarray:
        """One field in this set's layout in its storage type (after a device synchronise): block layout
        (nblocks,) + shape(name), LAYOUT_LEVELS shape(name)."""
        self.hip.hipSetDevice(self.device)
        self.hip.hipDeviceSynchronize()
        dt = np.int32 if name == "ktype" else storage_dtype(self.precision)
        if self._layout() == LAYOUT_LEVELS:
            out = np.empty(self.shape(name), dtype=dt)
        else:
            out = np.empty((nblocks_of(self.ngptot, self.nproma),) + self.shape(name), dtype=dt)
        rc = self.hip.hipMemcpy(out.ctypes.data, getattr(self.f, name), out.nbytes, 2)
        if rc != 0:
            raise CloudscError("hipMemcpy %s failed (%d)" % (name, rc))
        return out

    def download(self, name: str) -> np.ndarray:
        """One field in this set's layout as float64."""
        return self.download_raw(name).astype(np.float64)

    def close(self) -> None:
        if getattr(self, "f", None) is not None:
            if getattr(self, "tend_planes", 0):   # the separate arrays back, the buffers freed
                for b in (self.buffer_tmp, self.buffer_loc):
                    self.hip.hipFree(b)
                C.memmove(C.byref(self.f), C.byref(self.separate), C.sizeof(Fields))
                self.tend_planes = 0
            self.lib.cloudsc_fields_free(self.device, C.byref(self.f))
            self.f = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
