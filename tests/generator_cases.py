"""The instance generator's configuration space: sixteen configurations that reach what c2 .. c5 and the small grids do
not (64-lane groups chosen by the configuration, the knobs at their ends, 16-pin nets, 1x1 and fully pinned components,
different w and h ranges on non-square grids, streams the reference itself stops on), the fixture the reference recorded for them
(tests/golden/generator_tables.npz, written by make_golden.record_generator_tables) and the host twin driven stream by
stream.  Shared by the CPU tests (test_host_logic.py, test_instance_gen_native.py) and tests/test_device_generator_gpu.py.
A plain module: nothing here touches a device."""
import ctypes as C
import os

import numpy as np

from pcbenv import EnvConfig
from pcbenv.instances import instance_stride, unpack_instances

TAIL = ("centroid", 2, 0.5)
# name -> (kind, constructor arguments in the reference's order, lanes per environment gen_group_lanes must choose)
CASES = {
    "pin_knobs00": ("pin", (64, 64, 0, 0, 2, 6, 2, 6, 16, 16, 8, 8, 6, 6) + TAIL, 16),          # sigma = 1, kcomp floor of the pin kind
    "spatial_dist0": ("spatial", (64, 64, 0, 9, 2, 6, 2, 6, 16, 10, 4, 8, 6, 2) + TAIL, 16),
    "spatial_spread0": ("spatial", (64, 64, 9, 0, 2, 6, 2, 6, 16, 10, 4, 8, 6, 2) + TAIL, 16),  # kcomp = 1, k grows one by one
    "pin_g32": ("pin", (64, 64, 1, 5, 2, 6, 2, 6, 24, 10, 4, 12, 8, 2) + TAIL, 32),             # pin kind at G = 32
    "spatial_max": ("spatial", (128, 128, 9, 9, 2, 8, 2, 8, 64, 40, 8, 16, 16, 4) + TAIL, 64),  # 64 components, <= 256 pins, 16-pin nets
    "pin_wide": ("pin", (128, 128, 2, 3, 2, 8, 2, 8, 64, 33, 8, 16, 16, 4) + TAIL, 64),         # pin-kind ids at G = 64
    "spatial_32nets": ("spatial", (48, 48, 4, 4, 1, 8, 1, 8, 40, 20, 10, 32, 8, 2) + TAIL, 64),  # 32 nets, 1x1 .. 8x8 components
    "pin_tiny_full": ("pin", (12, 12, 7, 2, 1, 2, 1, 2, 10, 5, 1, 3, 4, 2) + TAIL, 16),         # 1x1 components, every cell pinned
    "rect_wide": ("rect", (33, 65, 1, 9, 1, 9, 40, 5), 64),                                     # rect kind at G = 64
    "fail_pin": ("pin", (10, 10, 5, 5, 2, 4, 2, 4, 4, 1, 1, 3, 6, 4) + TAIL, 16),               # about half of the streams stop
    "fail_spatial_1x1": ("spatial", (8, 8, 5, 5, 1, 2, 1, 2, 3, 1, 1, 2, 3, 1) + TAIL, 16),     # streams stop on num_nets < 1
    "fail_nets16": ("spatial", (24, 24, 5, 5, 2, 4, 2, 4, 12, 6, 2, 3, 16, 16) + TAIL, 16),     # about 15 % stop; 16-pin nets
    # different w and h ranges on H != W (arguments: ..., min_w, max_w, min_h, max_h, ...): a swapped axis shows here
    "pin_asym_40x72": ("pin", (40, 72, 5, 5, 2, 8, 2, 4, 12, 8, 4, 6, 6, 3) + TAIL, 16),
    "spatial_asym_72x40": ("spatial", (72, 40, 5, 5, 2, 4, 2, 8, 12, 8, 4, 6, 6, 3) + TAIL, 16),
    "spatial_asym_9x14": ("spatial", (9, 14, 3, 4, 2, 5, 1, 3, 6, 2, 2, 4, 5, 2) + TAIL, 16),
    "rect_asym_12x7": ("rect", (12, 7, 2, 3, 1, 5, 6, 2), 16),
}
FAIL_CASES = tuple(n for n in CASES if n.startswith("fail_"))
OK_CASES = tuple(n for n in CASES if not n.startswith("fail_"))
ASYM_CASES = tuple(n for n in CASES if "_asym_" in n)
RESETS = 8            # records per stream in the fixture
NEVER = 1 << 30       # fail_at of a stream that does not stop
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generator_tables.npz")
_MAKE = {"rect": EnvConfig.rect, "pin": EnvConfig.pin, "spatial": EnvConfig.spatial}
PIN_FIELDS = ("pin_rel_x", "pin_rel_y", "pin_net", "pin_comp", "pin_id")


def make_cfg(name):
    kind, args, _ = CASES[name]
    return _MAKE[kind](*args)


def group_lanes(cfg, forced=0):
    """gen_group_lanes of csrc/pcb_geninst.h restated: lanes per environment of the generator kernel."""
    c, n, p = cfg.max_num_components, cfg.max_num_nets, cfg.max_total_pins
    g = 16 if (c <= 16 and n <= 16 and p <= 64) else 32 if (c <= 32 and n <= 32 and p <= 128) else 64
    return forced if forced in (32, 64) and forced > g else g


def instance_tables(ins):
    """One Instance as the fixture keeps a record: (comp [ncomp, 2] = h, w; num_nets; pins [npins, 5] = PIN_FIELDS)."""
    comp = np.stack([np.asarray(ins.comp_h, np.int64), np.asarray(ins.comp_w, np.int64)], axis=1)
    pins = np.stack([np.asarray(getattr(ins, f), np.int64) for f in PIN_FIELDS], axis=1) if ins.num_pins else np.zeros((0, 5), np.int64)
    return comp, int(ins.num_nets), pins


def load_fixture(name):
    """-> [(seed, records, fail_at, exception class name)]: `records` are the (comp, num_nets, pins) tables of the
    stream's resets before the one the reference raised on (fail_at = NEVER, "": all RESETS of them)."""
    z = np.load(FIXTURE)
    seeds, fail_at, exc = z[name + "/seeds"], z[name + "/fail_at"], z[name + "/fail_exc"]
    ncomp, nnets, npins = z[name + "/ncomp"], z[name + "/nnets"], z[name + "/npins"]
    comp, pins = z[name + "/comp_hw"].astype(np.int64), z[name + "/pins"].astype(np.int64)
    out, ci, pi = [], 0, 0
    for s in range(len(seeds)):
        good = RESETS if fail_at[s] < 0 else int(fail_at[s])
        recs = []
        for r in range(good):
            nc, np_ = int(ncomp[s, r]), int(npins[s, r])
            recs.append((comp[ci:ci + nc], int(nnets[s, r]), pins[pi:pi + np_]))
            ci, pi = ci + nc, pi + np_
        assert (ncomp[s, good:] == -1).all()
        out.append((int(seeds[s]), recs, NEVER if fail_at[s] < 0 else good, str(exc[s])))
    assert ci == len(comp) and pi == len(pins)
    return out


def same_tables(got, want):
    return np.array_equal(got[0], want[0]) and got[1] == want[1] and np.array_equal(got[2], want[2])


def native_stream(cfg, seed, n):
    """n calls of pcbenv_instgen_next on one stream of the host twin (csrc/instance_gen.cpp) -> (packed records
    uint8 [n, stride], fail_at, code): the stream is not advanced past the first record it cannot generate, whose index
    is fail_at (NEVER: none) and whose return code is `code`; the rows from fail_at on stay zero."""
    from pcbenv import _lib
    L = _lib.load()
    ccfg = _lib.make_config(cfg, 1)
    h = C.c_void_p()
    _lib.check(L.pcbenv_instgen_create(C.byref(ccfg), int(seed), C.byref(h)))
    out = np.zeros((n, instance_stride(cfg)), np.uint8)
    fail_at, code = NEVER, 0
    try:
        for r in range(n):
            code = int(L.pcbenv_instgen_next(h, C.c_void_p(out[r].ctypes.data)))
            if code != 0:
                out[r] = 0
                fail_at = r
                break
    finally:
        L.pcbenv_instgen_destroy(h)
    return out, fail_at, code


def native_streams(cfg, seeds, n):
    """native_stream for every seed -> (records uint8 [n, len(seeds), stride], fail_at int64 [len(seeds)])."""
    recs = np.zeros((n, len(seeds), instance_stride(cfg)), np.uint8)
    fail_at = np.full(len(seeds), NEVER, np.int64)
    for i, s in enumerate(seeds):
        recs[:, i], fail_at[i], _ = native_stream(cfg, s, n)
    return recs, fail_at


def packed_tables(cfg, rec):
    return instance_tables(unpack_instances(cfg, rec[None])[0])
