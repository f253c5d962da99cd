"""The field inventory (csrc/cloudsc_fields.def) against everything that is
not generated from it: the hand-written public header, the ctypes mirror in
cloudsc_amd.py and the tables libcloudsc_io.so exports -- and, member by
member, which fields an entry point requires (fields_complete).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cloudsc_amd as ca

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "cloudsc_amd.h")
INVENTORY = os.path.join(REPO, "dwarf-p-cloudsc_amd", "csrc", "cloudsc_fields.def")
IO_LIB = os.path.join(os.path.dirname(ca.LIB_PATH), "libcloudsc_io.so")

KIND = {"LEVEL": "2d", "HALF": "2dh", "SPECIES": "3d", "SURFACE": "1d"}
KIND_CODE = {"LEVEL": 0, "HALF": 1, "SPECIES": 2, "SURFACE": 3}
DIRECTION = {"IN": ca.INPUT_FIELDS, "AEROSOL": ca.AEROSOL_FIELDS, "INOUT": ca.INOUT_FIELDS, "OUT": ca.OUTPUT_FIELDS}


def uncommented(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def macro_body(text, name):
    """The continued lines of `#define name(X) ...`."""
    m = re.search(r"#define %s\(X\)((?:.*\\\n)*.*)\n" % name, text)
    assert m, name
    return m.group(1)


def inventory():
    text = uncommented(INVENTORY)
    rows = re.findall(r"X\((\w+), (\w+), (\w+), (\w+), ([01])\)", macro_body(text, "CLOUDSC_FIELDS"))
    template = re.findall(r"X\((\w+)\)", macro_body(text, "CLOUDSC_TEMPLATE_ORDER"))
    validated = re.findall(r'X\((\w+), "([^"]+)"\)', macro_body(text, "CLOUDSC_VALIDATED_ORDER"))
    return rows, template, validated


def struct_members(text, name):
    """Pointer members of `typedef struct ... { ... } name;`, in order."""
    body = re.search(r"\{([^{}]*)\}\s*%s\s*;" % name, text).group(1)
    return re.findall(r"\*\s*(\w+)", body)


ROWS, TEMPLATE, VALIDATED = inventory()
REQUIRED = [n for n, _, _, d, _ in ROWS if d != "AEROSOL"]


def test_inventory_matches_header_and_ctypes_mirror():
    header = uncommented(HEADER)
    members = [r[0] for r in ROWS]
    assert len(members) == 48 and len(TEMPLATE) == 28 and len(VALIDATED) == 21
    assert members == struct_members(header, "cloudsc_fields_t")
    assert members == [n for n, _ in ca.Fields._fields_]
    assert TEMPLATE == struct_members(header, "cloudsc_template_t")
    assert TEMPLATE == [n for n, _ in ca.Template._fields_[2:]]
    enum = re.search(r"enum\s+cloudsc_field_id\s*\{([^}]*)\}", header).group(1)
    assert ["CLOUDSC_F_" + n for n, _ in VALIDATED] == re.findall(r"CLOUDSC_F_\w+", enum)
    by_dataset = {N: n for n, N, _, _, _ in ROWS}
    assert [(p, by_dataset[N]) for N, p in VALIDATED] == ca.VALIDATED
    # the template and the validated order hold exactly the rows of their directions
    assert sorted(TEMPLATE) == sorted(n for n, _, _, d, _ in ROWS if d != "OUT")
    assert sorted(N for N, _ in VALIDATED) == sorted(N for _, N, _, d, _ in ROWS if d in ("INOUT", "OUT"))


def test_inventory_kinds_and_directions_match_python():
    assert [n for n, _, _, _, _ in ROWS] == list(ca.ALL_FIELDS)
    for n, N, kind, direction, is_int in ROWS:
        assert N == n.upper()
        assert ca.ALL_FIELDS[n] == KIND[kind], n
        assert [d for d, fields in DIRECTION.items() if n in fields] == [direction], n
        assert (is_int == "1") == (n == "ktype"), n
    for direction, fields in DIRECTION.items():          # key order of the four dicts: member order
        assert list(fields) == [n for n, _, _, d, _ in ROWS if d == direction]


def test_io_library_tables_match_inventory():
    if not os.path.exists(IO_LIB):
        pytest.skip("libcloudsc_io.so not built (__graft_entry__.build())")
    io = C.CDLL(IO_LIB)
    row = {n: r for r in ROWS for n in (r[0], r[1])}     # by member and by dataset name

    def names(symbol, n):
        return [s.decode() for s in (C.c_char_p * n).in_dll(io, symbol)]

    def kinds(symbol, n):
        return list((C.c_int * n).in_dll(io, symbol))

    assert names("cloudsc_io_input_names", 28) == [row[n][1] for n in TEMPLATE]
    assert kinds("cloudsc_io_input_kind", 28) == [KIND_CODE[row[n][2]] for n in TEMPLATE]
    assert names("cloudsc_io_ref_names", 21) == [N for N, _ in VALIDATED]
    assert names("cloudsc_io_print_names", 21) == [p for _, p in VALIDATED]
    assert kinds("cloudsc_io_ref_kind", 21) == [KIND_CODE[row[N][2]] for N, _ in VALIDATED]


# ---------------------------------------------------------------------------
# required and optional members of cloudsc_fields_t
# ---------------------------------------------------------------------------
NGPTOT, NPROMA, KLEV = 3, 2, 2      # the smallest klev accepted; a partial last block


@pytest.fixture(scope="module")
def tiny(ds):
    """Every field backed by host arrays: the top KLEV levels of the dataset's
    inputs in block layout, ones for the aerosol inputs, NaN outputs."""
    if not os.path.exists(ca.LIB_PATH):
        pytest.skip("libcloudsc_amd.so not built (__graft_entry__.build())")
    cut = {"2d": lambda a: a[:KLEV], "2dh": lambda a: a[:KLEV + 1], "3d": lambda a: a[:, :KLEV], "1d": lambda a: a}
    arrays = {}
    for n, kind in ca.ALL_FIELDS.items():
        shape = (ca.nblocks_of(NGPTOT, NPROMA),) + ca.field_shape(kind, KLEV, NPROMA)
        if n in ds.inputs:
            dt = np.int32 if n == "ktype" else np.float64
            arrays[n] = ca.expand(cut[kind](ds.inputs[n]), kind, NGPTOT, NPROMA, dtype=dt)
        else:
            arrays[n] = np.ones(shape) if n in ca.AEROSOL_FIELDS else np.full(shape, np.nan)
        assert arrays[n].shape == shape and arrays[n].flags["C_CONTIGUOUS"], n
    lib = ca.gpu_lib()
    plude0 = arrays["plude"].copy()

    def run(null=(), **params):
        arrays["plude"][...] = plude0                     # INOUT
        p = ca.Params.from_dict(dict(ds.params, **params))
        f = ca.Fields()
        for n in ca.ALL_FIELDS:
            setattr(f, n, None if n in null else arrays[n].ctypes.data)
        return lib.cloudsc_cpu_run(1, NGPTOT, NPROMA, KLEV, C.byref(p), C.byref(f), None)

    return run


def test_cpu_run_accepts_every_field_set(tiny):
    assert len(REQUIRED) == 43
    assert tiny() == 0
    assert tiny(laericesed=1, laericeauto=1) == 0


@pytest.mark.parametrize("member", REQUIRED)
def test_cpu_run_requires_each_non_aerosol_member(tiny, member):
    assert tiny(null=(member,)) == ca.EINVAL


def test_cpu_run_aerosol_members_are_optional_until_read(tiny):
    assert tiny(null=tuple(ca.AEROSOL_FIELDS), laericesed=0, laericeauto=0) == 0
    assert tiny(null=("pre_ice",), laericesed=1) == ca.EINVAL
