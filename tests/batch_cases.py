"""TEST INFRASTRUCTURE ONLY -- the cases of the batched step (cloudsc_batch_create / cloudsc_gpu_run_batch), named
once: the smallest shapes at which the mapping member -> grid row, block -> workgroup, column -> lane can go wrong.

  shapes    (100, 32)  4 blocks, the last one 4 lanes wide; unpacked, and packed on request (2 blocks per wave);
            (40, 16)   3 narrow blocks: packed by default, 4 blocks per wave, so the one wave of a member has a
                       fourth sub-slot that lies in no block of that member -- it must not run into the next
                       member's first block; and unpacked;
            (64, 64)   one full wave per member;
  nsets     1, 2 and 3;
  states    the W and M golden scenarios at their own KLEV (137), W cut to KLEV 3 (NCLDTOP 2), W with aerosols
            (form_state_cases.py's states);
  precision fp64, fp32 and mixed; outputs ALL, PROGNOSTIC and SURFACE.

Set i of a case holds the state's columns from column i * OFFSET on (the template wraps), so no two sets of a batch
hold the same inputs: a member run with another member's table entry shows.  Nothing here calls the library under
test."""
import cloudsc_amd as ca

CANARY = 0xC3                       # every byte of every output before a run
OFFSET = 37                         # set i starts at template column i * OFFSET (of 100)

# (ngptot, nproma, narrow_pack mode, blocks per wave expected)
SHAPES = [(100, 32, 0, 1), (100, 32, 1, 2), (40, 16, -1, 4), (40, 16, 0, 1), (64, 64, -1, 1)]
PRECISIONS = {"fp64": ca.FP64, "fp32": ca.FP32, "mixed": ca.MIXED}
OUTPUTS = {"all": ca.OUTPUTS_ALL, "prognostic": ca.OUTPUTS_PROGNOSTIC, "surface": ca.OUTPUTS_SURFACE}
NSETS = (1, 2, 3)
STATES = ("W", "M", "klev3")
AEROSOL_STATE = "aerosol_W"


def _table():
    """Every (shape, precision, outputs); nsets and the state cycle so that each value of either meets every
    shape, every precision and every selection."""
    out = []
    for i, shape in enumerate(SHAPES):
        for j, prec in enumerate(PRECISIONS):
            for k, outs in enumerate(OUTPUTS):
                out.append((STATES[(i + j + k) % 3], NSETS[(i + 2 * j + k) % 3]) + shape + (prec, outs))
    # aerosols: per batch all sets or none -- packed and unpacked, every precision
    for j, prec in enumerate(PRECISIONS):
        out.append((AEROSOL_STATE, 2, 40, 16, -1, 4, prec, "all"))
        out.append((AEROSOL_STATE, 3, 100, 32, 0, 1, prec, "surface" if j else "prognostic"))
    return out


CASES = _table()


def case_id(c):
    state, nsets, ngptot, nproma, pack, _, prec, outs = c
    return "%s-n%d-%dx%d-%s-%s-%s" % (state, nsets, ngptot, nproma, {0: "unpacked", 1: "packed", -1: "default"}[pack],
                                     prec, outs)


def perturbed_params(params):
    """Three parameter sets for "one state, N parameter sets": the state's own, and two with RAMID and RCLDIFF
    changed (the cloud fraction threshold of the ice phase and the erosion coefficient: both act at every cloudy
    level, so every set's tendencies differ)."""
    a, b = dict(params), dict(params)
    a["ramid"], a["rcldiff"] = params["ramid"] * 0.75, params["rcldiff"] * 2.0
    b["ramid"], b["rcldiff"] = params["ramid"] * 1.125, params["rcldiff"] * 0.5
    return [dict(params), a, b]
