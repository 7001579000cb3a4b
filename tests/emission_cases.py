"""Cases, a placed allocator and the branch predicates of the observation emission (plain module, no test; needs no GPU).

Every observation byte leaves the device through emit_plane_ / emit_plane2_ / emit_zero_ (csrc/pcb_team_io.h),
emit_pin_grid / emit_component_grid_to / feat_cache_emit / emit_features_* (csrc/pcb_observe.h) and store16_or_tail
(csrc/pcb_env_lds.h), which branch on the shape, on the address the caller bound and -- with
PCBENV_FLAG_INCREMENTAL_OBS -- on the rows [r0, r1) of the placement.  This module holds

  PlacedAllocator  the `allocator=` of BatchedPlacementEnv: every tensor is a view into a sentinel-filled uint8 buffer, a
                   guard in front and behind, a per-tensor misplacement, the interior left dirty;
  paths            the branch predicates restated in plain Python, one function per emission routine, each citing the
                   line it restates: (configuration, layout, placement) -> the set of labels a run reaches;
  CASES            the table: configuration, handle keywords, offsets, B, seed, script.

`Plan` computes a case's script on the CPU before any device call -- a HandleModel stepped with the actions the sampling
contract draws (rollout_cases.draws), a few corrupted -- so the rows [r0, r1) of every step, the pins of every instance
and the terminals exist beforehand; tests/test_emission_cases.py asserts on the plans alone that the table reaches every
label of LABELS, tests/test_emission_gpu.py runs the same plans on the device.
"""
import zlib
from functools import lru_cache

import numpy as np

from pcbenv import EnvConfig, named_config
from pcbenv.config import KIND_PIN, KIND_RECT, KIND_SPATIAL, KIND_SQUARE

import playout_cases as pc
import rollout_cases as rc
from handle_model import HandleModel
from logits_cases import RAGGED

SENTINEL = 0xA5   # no legal value of a cell tensor (0 / 1) or a compact feature (-1 .. 127, ids < 256 * 64); as int8 -91,
                  # as int16 -23131, as float64 -1.2e-130: no feature value either
GUARD = 256       # bytes in front of and behind every tensor
CELL_KEYS = ("grid", "action_mask", "pin_grid", "component_grid")
KIND_NAME = {KIND_SQUARE: "square", KIND_RECT: "rect", KIND_PIN: "pin", KIND_SPATIAL: "spatial"}
POLICIES = {"default": None, "stream": {"stream_threshold_bytes": 0}}
STREAM_THRESHOLD_DEFAULT = 256 << 20  # csrc/pcb_config.hip:94


# ---------------------------------------------------------------------------------------------------------------------
# a. the placed allocator
# ---------------------------------------------------------------------------------------------------------------------
class PlacedAllocator:
    """`f(name, shape, dtype)` for BatchedPlacementEnv(allocator=...).  Tensor `name` is a view that starts
    guard + offset(name) bytes into a uint8 buffer of its own, filled with SENTINEL, with `guard` bytes behind it.
    offsets: the misplacement of the cell tensors (grid, action_mask, pin_grid, component_grid), 0 where not given; a
    feature tensor is misplaced by its element size.  The buffers are kept: `snapshot()` is one device -> host copy each."""

    def __init__(self, offsets=None, device="cuda:0", guard=GUARD):
        assert guard >= 256
        self.offsets, self.device, self.guard = dict(offsets or {}), device, guard
        self.backing, self.where = {}, {}

    def offset(self, name, itemsize):
        return int(self.offsets.get(name, 0)) if name in CELL_KEYS else int(itemsize)

    def __call__(self, name, shape, dtype):
        import torch
        item = torch.empty((), dtype=dtype).element_size()
        n = int(np.prod(shape)) * item
        start = self.guard + self.offset(name, item)
        total = start + n + self.guard
        raw = torch.full((total + 255,), SENTINEL, dtype=torch.uint8, device=self.device)
        shift = -raw.data_ptr() % 256  # the buffer itself adds no misplacement, whatever the device's allocator aligns to
        buf = raw[shift:shift + total]
        assert buf.data_ptr() % 256 == 0
        self.backing[name] = buf
        self.where[name] = (start, n, tuple(shape), torch.empty(0, dtype=dtype).numpy().dtype)
        return buf[start:start + n].view(dtype).view(tuple(shape))

    def snapshot(self):
        """name -> (front guard, interior, back guard), uint8 host copies of one transfer per buffer."""
        out = {}
        for name, buf in self.backing.items():
            start, n, _, _ = self.where[name]
            h = buf.cpu().numpy()
            out[name] = (h[:start], h[start:start + n], h[start + n:])
        return out

    def typed(self, name, interior):
        """An interior of snapshot() in the tensor's shape and dtype."""
        _, _, shape, dtype = self.where[name]
        return interior.view(dtype).reshape(shape)

    def dirty(self, slot):
        """Slot `slot` of every tensor back to the sentinel."""
        for name, buf in self.backing.items():
            start, n, shape, _ = self.where[name]
            per = n // shape[0]
            buf[start + slot * per:start + (slot + 1) * per] = SENTINEL


# ---------------------------------------------------------------------------------------------------------------------
# b. the branch predicates
# ---------------------------------------------------------------------------------------------------------------------
class Layout:
    """What the predicates need of a handle besides its configuration: the handle keywords, the offsets of the cell
    tensors, B and the store policy (the value of stream_threshold_bytes, None = the default)."""

    def __init__(self, cfg, kw, offsets, B, stream_threshold=None):
        k = cfg.kind
        pins = k in (KIND_PIN, KIND_SPATIAL)
        self.cfg, self.kind, self.B, self.offsets = cfg, k, B, dict(offsets or {})
        self.H, self.W, self.WW, self.O = cfg.height, cfg.width, (cfg.width + 63) // 64, cfg.num_orientations
        self.C = 0 if k == KIND_SQUARE else cfg.max_num_components                      # csrc/pcb_config.hip:81-87
        self.K = cfg.max_num_nets + 1 if pins else 1
        self.mp = cfg.max_component_h * cfg.max_component_w
        self.F = 5 + self.mp if k == KIND_SPATIAL else 5
        t = kw.get("threads_per_env", 0)                                                # csrc/pcb_config.hip:111-112
        self.threads = t if t in (64, 256) else (256 if self.H * self.W * (self.K + 5 if k == KIND_SPATIAL else 5) > 64 * 1024 else 64)
        self.NW = self.threads // 64
        self.routes = pins and cfg.reward_type != "centroid"                            # pcb_layout::routes_compiled_in
        self.S = kw.get("num_slots", 1)
        self.inc, self.compact = bool(kw.get("incremental_obs")), bool(kw.get("compact_features"))
        self.auto_reset = bool(kw.get("auto_reset"))
        self.cg_total = self.C * self.mp * self.K
        # csrc/pcb_config.hip:93, csrc/pcb_host.h:85, dispatch_step (csrc/pcbenv_api.hip): the bytes of every slot against the threshold
        cells = self.H * self.W
        per_env = cells * self.O if self.inc else cells * (1 + self.O + (self.K if k == KIND_SPATIAL else 0))
        self.stream = per_env * B * self.S > (STREAM_THRESHOLD_DEFAULT if stream_threshold is None else stream_threshold)
        self.cells_aligned16 = all(self.offsets.get(n, 0) % 16 == 0 for n in ("grid", "action_mask", "pin_grid"))  # pcbenv_bind_buffers_slots

    def off(self, name):
        return self.offsets.get(name, 0)


def fixed_geometry_applies(L, enabled=True, num_steps=1):
    """pcb_layout::fixed_geometry_applies (csrc/pcb_layout.h)."""
    return (enabled and L.kind in (KIND_PIN, KIND_SPATIAL) and not L.routes and L.H == 64 and L.W == 64 and L.O == 4 and L.WW == 1
            and L.threads // 64 == 1 and L.S == 1 and num_steps == 1 and L.cells_aligned16)


def fold_across_lanes(WW, threads, H):
    """pcb_layout::fold_across_lanes (csrc/pcb_layout.h)."""
    return WW == 1 and threads == 64 and H <= 64


def member_words(kind, C, mp):
    """pcb_layout::member_words (csrc/pcb_layout.h)."""
    return (C * mp + 63) // 64 if kind == KIND_PIN else 0


def plane_arm(L, base):
    """csrc/pcb_team_io.h:33 emit_plane_ (and :59 emit_plane2_, whose two destinations lie 2 * H * W apart): the arm a
    plane at byte address `base` (modulo 16) takes."""
    W = L.W
    if W % 16 == 0 and base % 16 == 0:
        return "vector/pow2" if W & (W - 1) == 0 else f"vector/npow2/WW{L.WW}"       # :35 `sh`
    return "byte/W%16" if W % 16 else "byte/misaligned"                               # :41


def plane_paths(L, row, r0, r1, fixed):
    """grid rows [r0, r1) and the action_mask planes of output row `row`: csrc/pcb_observe.h:60 mask_and_emit."""
    HW, out = L.H * L.W, set()
    arm = plane_arm(L, L.off("grid") + row * HW)                                      # :64 the grid, through emit_plane_
    out.add("plane:" + arm)
    if (r0, r1) != (0, L.H) and arm.startswith("vector"):
        out.add("plane:" + arm + "/partial")
    m = L.off("action_mask") + row * L.O * HW
    if L.kind in (KIND_PIN, KIND_SPATIAL):                                            # :76, :88 emit_plane2_(m + o * HW, m + (o + 2) * HW)
        for o in (0, 1):
            arm = plane_arm(L, m + o * HW)
            out.add("plane2:" + arm)
            if arm.startswith("vector") and fixed:
                out.add("plane2:vector/fixed64")                                      # csrc/pcb_team_io.h:66 the trips written out
            if arm.startswith("byte"):
                out.add("plane:" + arm)                                               # csrc/pcb_team_io.h:85 falls back to emit_plane_ twice
    else:
        for o in range(L.O):                                                          # :68, :76 emit_plane_ per plane
            out.add("plane:" + plane_arm(L, m + o * HW))
    out.add("mask:fold/lanes" if fold_across_lanes(L.WW, L.threads, L.H) else "mask:fold/lds")  # csrc/pcb_team_io.h:105
    return out


def pin_grid_out_arm(L, row, r0, r1):
    """csrc/pcb_observe.h:124: 16-byte chunks or bytes."""
    b0, b1, base = r0 * L.W * L.K, r1 * L.W * L.K, L.off("pin_grid") + row * L.H * L.W * L.K
    if b0 % 16 == 0 and b1 % 16 == 0 and base % 16 == 0:
        return "chunks"
    return "byte/b0b1" if (b0 % 16 or b1 % 16) else "byte/misaligned"


def pin_grid_paths(L, row, r0, r1):
    """csrc/pcb_observe.h:98 emit_pin_grid, rows [r0, r1) of output row `row`."""
    K = L.K
    out = {"pin_grid:cls/16cells" if L.W % 16 == 0 else "pin_grid:cls/byte"}            # :104
    arm = pin_grid_out_arm(L, row, r0, r1)
    if arm == "chunks":
        out.add("pin_grid:out/chunks/" + ("K>=8" if K >= 8 else "5<=K<8" if K >= 5 else "K<5"))  # :141, :161
        if K in (2, 33):
            out.add(f"pin_grid:out/chunks/K={K}")
    else:
        out.add("pin_grid:out/" + arm)                                                 # :164
    return out


def zero_paths(L, row):
    """csrc/pcb_team_io.h:48 emit_zero_ over pin_grid at a reset (csrc/pcb_reset.h:246)."""
    n = L.H * L.W * L.K
    return {"zero:vector" if n % 16 == 0 and (L.off("pin_grid") + row * n) % 16 == 0 else "zero:byte"}


def component_grid_paths(L, row, source):
    """csrc/pcb_observe.h:200 emit_component_grid_to (source "tables") and :272 feat_cache_emit (source "cache"), with
    csrc/pcb_env_lds.h:52 store16_or_tail."""
    total, base = L.cg_total, L.off("component_grid") + row * L.cg_total
    if total % 4 == 0 and base % 4 == 0:
        if total % 16 == 0:
            return {f"cg:{source}:chunks/notail"}
        out = {f"cg:{source}:chunks/tail"}                                             # the last chunk dword by dword
        if base % 16:
            out.add(f"cg:{source}:chunks/tail/base4only")
        return out
    return {f"cg:{source}:byte/" + ("total%4" if total % 4 else "misaligned")}


def feature_paths(L, whole):
    """The feature tensors of one environment: whole (csrc/pcb_observe.h:367 emit_features_full, :288 _compact) or row-wise
    (csrc/pcb_reset.h:182); the (component, field) advance of all_components_feature carries where C * F exceeds the team."""
    out = set()
    if L.kind == KIND_SQUARE:
        return out
    if whole:
        out.add("feat:whole/compact" if L.compact else "feat:whole/f64")
    out.add("feat:CF>NT" if L.C * L.F > L.threads else "feat:CF<=NT")                  # csrc/pcb_observe.h:374-389, csrc/pcb_reset.h:188-203
    return out


def reset_paths(L, row, first, npins):
    """csrc/pcb_reset.h:23 reset_env of one environment into output row `row`: `first` = its first reset since the bind,
    npins = the pins of the instance it takes."""
    out = plane_paths(L, row, 0, L.H, False)
    full = L.S > 1                                                                     # :26
    out |= feature_paths(L, full)
    if L.kind in (KIND_PIN, KIND_SPATIAL) and not full:
        out.add("feat:rowwise/first-reset-zero-fill" if first else "feat:rowwise/rows_cleared")  # :43, :217-229
    if L.kind == KIND_PIN:
        out.add("feat:pin-q1/np<=64" if npins <= 64 else "feat:pin-q1/np>64")          # :109, :120
        out.add("feat:pin/member_words=1" if member_words(L.kind, L.C, L.mp) == 1 else "feat:pin/member_words>1")
    if L.kind == KIND_SPATIAL:
        out.add("feat:spatial-rank/np<=64" if npins <= 64 else "feat:spatial-rank/np>64")  # :156, :166
        out |= zero_paths(L, row) | component_grid_paths(L, row, "tables")             # :246, :247
    return out


def whole_paths(L, row):
    """Every tensor of output row `row` from the state in LDS: k_gather (csrc/pcb_kernels.h:62-70) and the step of the
    trajectory layout that cannot copy from the cache (csrc/pcb_step.h:146-148, :160-164)."""
    out = plane_paths(L, row, 0, L.H, False) | feature_paths(L, True)
    if L.kind == KIND_SPATIAL:
        out |= component_grid_paths(L, row, "tables") | pin_grid_paths(L, row, 0, L.H)
    return out


STEP_BUILDS = ("inplace", "inplace_stream", "slot", "rollout")  # STEP_BUILD_* of csrc/pcb_layout.h, by value


def step_build(L, num_steps=1, enabled=True):
    """The k_step instantiation of a launch of num_steps transitions: pcb_layout::select_step_build (csrc/pcb_layout.h)
    -> (WW, NW, routes, BUILD, fixed)."""
    traj = L.S > 1 or num_steps > 1
    build = ("slot" if num_steps == 1 else "rollout") if traj else ("inplace_stream" if L.stream else "inplace")
    return L.WW, L.NW, L.routes, build, fixed_geometry_applies(L, enabled, num_steps)


def step_build_part(kind, build):
    """The translation unit that compiles a build: pcb_layout::step_build_part (csrc/pcb_layout.h); None = no unit does."""
    WW, NW, routes, name, fixed = build
    pins = kind in (KIND_PIN, KIND_SPATIAL)
    if fixed:
        return 4 if pins and not routes and WW == 1 and NW == 1 and name in ("inplace", "inplace_stream") else None
    if routes:
        return (2 if NW == 1 else 3) if pins else None
    return 1 if pins and name == "slot" else 0


def build_paths(L, name=""):
    build, fixed = step_build(L)[3:]
    kind = KIND_NAME[L.kind]
    out = {f"build:BUILD={build}", f"build:kind={kind}", f"build:WW={L.WW}", f"build:NW={L.NW}"}
    if L.kind in (KIND_PIN, KIND_SPATIAL):
        out.add(f"build:routes={'on' if L.routes else 'off'}/{kind}")
    if build == "inplace_stream":  # a separate instantiation per kind, WW and NW
        out |= {f"build:inplace_stream/WW={L.WW}", f"build:inplace_stream/NW={L.NW}", f"build:inplace_stream/kind={kind}"}
    if fixed:
        out.add("build:geo64")
    elif fixed_geometry_applies(Layout(L.cfg, {"threads_per_env": L.threads, "num_slots": L.S}, {}, L.B)):
        out.add("build:geo64-refused/" + ("c3" if L.kind == KIND_PIN else "c4"))       # misaligned cell tensors alone refuse it
    return out


def instantiation(L):
    """The kernel a step launch of this layout runs, by name."""
    build, fixed = step_build(L)[3:]
    return f"k_step<{KIND_NAME[L.kind]}, WW={L.WW}, NW={L.NW}, routes={int(L.routes)}, {build}{', geo64' if fixed else ''}>"


def paths(cfg, layout, placement):
    """The labels a run of `placement` -- the events of a Plan -- reaches on a handle of `cfg` laid out as `layout`."""
    L = layout
    assert L.cfg == cfg
    out = build_paths(L)
    fixed = step_build(L)[4]
    arms = {}  # (environment, episode) -> the pin_grid output arms of its incremental steps
    for ev in placement:
        s = ev["slot"]
        if ev["op"] == "reset":
            out.add("build:k_reset/masked" if ev["masked"] else "build:k_reset/whole")
            for e in ev["rows"]:
                out |= reset_paths(L, s * L.B + e, ev["first"][e], ev["npins"][e])
        elif ev["op"] == "gather":
            out.add("build:k_gather")
            for e in ev["rows"]:
                out |= whole_paths(L, s * L.B + e)
        else:
            for e in range(L.B):
                row = s * L.B + e
                valid, last = ev["valid"][e], ev["placed_all"][e]
                if valid and not (L.auto_reset and last and L.kind != KIND_SQUARE):      # csrc/pcb_step.h:79, :128 skip_emit
                    r0, r1 = ev["range"][e] if L.inc else (0, L.H)                       # :127
                    out |= plane_paths(L, row, r0, r1, fixed)
                    if L.kind == KIND_SPATIAL:
                        out |= pin_grid_paths(L, row, r0, r1)                            # :154
                        if L.inc:
                            arms.setdefault((e, ev["episode"][e]), set()).add(pin_grid_out_arm(L, row, r0, r1) == "chunks")
                    if L.S > 1:                                                          # :135 slot_features
                        out |= feature_paths(L, True)
                        if L.kind == KIND_SPATIAL:                                       # :136 from_cache = feat_cache_valid
                            out |= component_grid_paths(L, row, "cache" if L.compact else "tables")
                elif not valid and L.S > 1 and not L.auto_reset:                         # :159 the unchanged observation, whole
                    out |= whole_paths(L, row)
                if ev["done"][e] and L.auto_reset:                                       # :175 the reset in the launch
                    out |= reset_paths(L, row, False, ev["npins_next"][e])
                if ev["worst"][e]:
                    out.add("cond:worst-case-terminal")
    if any(len(a) == 2 for a in arms.values()):
        out.add("pin_grid:both-arms-in-one-episode")
    return out


# the cells of the list the table has to reach
LABELS = tuple(
    ["plane:" + a for a in ("vector/pow2", "vector/npow2/WW1", "vector/npow2/WW2", "byte/W%16", "byte/misaligned",
                            "vector/pow2/partial", "vector/npow2/WW1/partial", "vector/npow2/WW2/partial")]
    + ["plane2:" + a for a in ("vector/pow2", "vector/npow2/WW1", "vector/npow2/WW2", "byte/W%16", "byte/misaligned", "vector/fixed64")]
    + ["mask:fold/lanes", "mask:fold/lds"]
    + ["pin_grid:" + a for a in ("cls/16cells", "cls/byte", "out/chunks/K>=8", "out/chunks/5<=K<8", "out/chunks/K<5", "out/chunks/K=2",
                                 "out/chunks/K=33", "out/byte/b0b1", "out/byte/misaligned", "both-arms-in-one-episode")]
    + ["zero:vector", "zero:byte"]
    + [f"cg:{s}:{a}" for s in ("tables", "cache") for a in ("chunks/notail", "chunks/tail", "chunks/tail/base4only", "byte/total%4", "byte/misaligned")]
    + ["feat:" + a for a in ("rowwise/first-reset-zero-fill", "rowwise/rows_cleared", "whole/f64", "whole/compact", "pin-q1/np<=64",
                             "pin-q1/np>64", "pin/member_words=1", "pin/member_words>1", "spatial-rank/np<=64", "spatial-rank/np>64",
                             "CF<=NT", "CF>NT")]
    + ["build:BUILD=" + b for b in ("inplace", "inplace_stream", "slot")]
    + ["build:kind=" + k for k in ("square", "rect", "pin", "spatial")]
    + ["build:WW=1", "build:WW=2", "build:NW=1", "build:NW=4"]
    + [f"build:routes={r}/{k}" for r in ("on", "off") for k in ("pin", "spatial")]
    + [f"build:inplace_stream/{a}" for a in ("WW=1", "WW=2", "NW=1", "NW=4", "kind=square", "kind=rect", "kind=pin", "kind=spatial")]
    + ["build:geo64", "build:geo64-refused/c3", "build:geo64-refused/c4", "build:k_reset/whole", "build:k_reset/masked", "build:k_gather"]
    + ["cond:worst-case-terminal"])


# ---------------------------------------------------------------------------------------------------------------------
# c. the case table
# ---------------------------------------------------------------------------------------------------------------------
_CROWDED = (12, 12, 5, 5, 2, 5, 2, 5, 8, 8, 3, 5, 7, 2)
SEEDS = (3, 2, 6)


def _small_spatial():
    return EnvConfig.spatial(10, 10, 3, 4, 2, 4, 2, 4, 6, 1, 2, 4, 5, 2, "both", 2, 0.5)


def _script(steps, auto_reset):
    """The calls behind the unmasked reset every handle starts with: `steps` transitions -- explicit with a few actions
    corrupted, fused, explicit as drawn, in turn -- with (manual reset only) a reset_done behind every third, a masked
    reset halfway and one gather_ at the end, one more transition behind it."""
    calls = []
    for t in range(steps):
        calls.append((("step", 0.12), ("fused",), ("step", 0.0))[t % 3])
        if t % 3 == 2 and not auto_reset:
            calls.append(("reset_done",))
        if t == steps // 2:
            calls.append(("reset_mask", 0.5))
    calls += [("gather",), ("fused",)]
    return tuple(calls)


class Case:
    """cfg: a constructor; kw: handle keywords (threads_per_env, incremental_obs, num_slots, compact_features,
    mask_marginals, auto_reset); offsets: the misplacement of the cell tensors; needs: the labels the case is in the table
    for -- the reach check asserts them at the case's seed."""

    def __init__(self, name, cfg, kw, offsets, B, steps, needs, seed=3):
        self.name, self.cfg, self.kw, self.offsets, self.B, self.steps, self.seed = name, cfg, dict(kw), dict(offsets), B, steps, seed
        self.needs = tuple(needs)
        self.S, self.Q = self.kw.get("num_slots", 1), 4
        self.script = _script(steps, bool(self.kw.get("auto_reset")))
        assert not (self.kw.get("incremental_obs") and (self.kw.get("auto_reset") or self.S > 1))

    def layout(self, policy="default"):
        opt = POLICIES[policy]
        return Layout(self.cfg(), self.kw, self.offsets, self.B, None if opt is None else opt["stream_threshold_bytes"])


_INC = {"incremental_obs": True}
CASES = {c.name: c for c in (
    # K = 4, component_grid 180 bytes per environment (% 16 == 4): the dword tail, odd environments 4-byte aligned only
    Case("sp14x32_tail", lambda: EnvConfig.spatial(14, 32, 5, 5, 2, 3, 2, 3, 5, 2, 1, 3, 5, 2, "centroid", 2, 0.5), {}, {"component_grid": 4}, 8, 9,
         ("cg:tables:chunks/tail", "cg:tables:chunks/tail/base4only", "pin_grid:out/chunks/K<5", "plane:vector/pow2", "zero:vector")),
    Case("sp14x32_tail_slots", lambda: EnvConfig.spatial(14, 32, 5, 5, 2, 3, 2, 3, 5, 2, 1, 3, 5, 2, "centroid", 2, 0.5),
         {"num_slots": 3, "compact_features": True, "auto_reset": True}, {"component_grid": 4}, 8, 9,
         ("cg:cache:chunks/tail", "cg:cache:chunks/tail/base4only", "feat:whole/compact", "build:BUILD=slot")),
    Case("sp14x32_cg_odd_slots", lambda: EnvConfig.spatial(14, 32, 5, 5, 2, 3, 2, 3, 5, 2, 1, 3, 5, 2, "centroid", 2, 0.5),
         {"num_slots": 3, "compact_features": True}, {"component_grid": 1}, 6, 7, ("cg:cache:byte/misaligned", "cg:tables:byte/misaligned")),
    # W = 48 (a multiple of 16, no power of two) on one word; the lowest K; component_grid 90 bytes: the byte arm
    Case("sp9x48_k2_inc", lambda: EnvConfig.spatial(9, 48, 5, 5, 2, 3, 2, 3, 5, 2, 1, 1, 6, 2, "centroid", 2, 0.5), _INC, {}, 8, 9,
         ("plane:vector/npow2/WW1", "plane:vector/npow2/WW1/partial", "plane2:vector/npow2/WW1", "pin_grid:out/chunks/K=2", "cg:tables:byte/total%4")),
    Case("sp9x48_k2_slots", lambda: EnvConfig.spatial(9, 48, 5, 5, 2, 3, 2, 3, 5, 2, 1, 1, 6, 2, "centroid", 2, 0.5),
         {"num_slots": 3, "compact_features": True, "auto_reset": True}, {}, 8, 9, ("cg:cache:byte/total%4", "pin_grid:out/chunks/K=2")),
    # W = 80: two words per row in the vector arm, routed, one and four wavefronts
    Case("sp20x80_beam_inc", lambda: EnvConfig.spatial(20, 80, 5, 5, 2, 5, 2, 3, 7, 3, 2, 6, 6, 2, "beam", 2, 0.5), _INC, {}, 8, 10,
         ("plane:vector/npow2/WW2", "plane:vector/npow2/WW2/partial", "plane2:vector/npow2/WW2", "pin_grid:out/chunks/5<=K<8",
          "build:routes=on/spatial", "build:inplace_stream/WW=2")),
    Case("sp20x80_beam_t256_slots", lambda: EnvConfig.spatial(20, 80, 5, 5, 2, 5, 2, 3, 7, 3, 2, 6, 6, 2, "beam", 2, 0.5),
         {"threads_per_env": 256, "num_slots": 3, "auto_reset": True, "mask_marginals": True}, {}, 8, 10,
         ("build:NW=4", "build:BUILD=slot", "feat:whole/f64", "cg:tables:byte/total%4")),
    # the highest K: one chunk of class map per row; eight or nine 3 x 3 components carry up to 81 pins: the rank loop with np > 64
    # and, in the same batch, the ballot with np <= 64
    Case("sp16x16_k33", lambda: EnvConfig.spatial(16, 16, 5, 5, 3, 3, 3, 3, 9, 8, 24, 32, 3, 2, "centroid", 2, 0.5), {}, {}, 8, 10,
         ("pin_grid:out/chunks/K=33", "feat:spatial-rank/np>64", "feat:rowwise/rows_cleared")),
    Case("sp16x16_k33_slots", lambda: EnvConfig.spatial(16, 16, 5, 5, 3, 3, 3, 3, 9, 8, 24, 32, 3, 2, "centroid", 2, 0.5),
         {"num_slots": 3, "compact_features": True, "auto_reset": True}, {"pin_grid": 4}, 8, 10,
         ("pin_grid:out/byte/misaligned", "feat:spatial-rank/np>64", "zero:byte")),
    # W * K = 72: whether a step's rows start and end on a 16-byte boundary depends on where the component went
    Case("crowded12_inc", lambda: EnvConfig.spatial(*_CROWDED, "both", 2, 0.5), _INC, {}, 12, 9,
         ("pin_grid:both-arms-in-one-episode", "pin_grid:out/byte/b0b1", "pin_grid:out/chunks/5<=K<8", "pin_grid:cls/byte", "plane:byte/W%16",
          "cond:worst-case-terminal")),
    # H * W * K = 500: the byte arms of pin_grid and of the zero fill in every environment but each fourth
    Case("small10_inc", _small_spatial, _INC, {}, 8, 8, ("zero:byte", "pin_grid:out/byte/b0b1", "cg:tables:chunks/notail")),
    Case("small10_slots", _small_spatial, {"num_slots": 3, "compact_features": True, "auto_reset": True}, {}, 8, 8,
         ("zero:byte", "pin_grid:out/byte/b0b1", "feat:whole/compact", "cg:cache:chunks/notail")),
    # two words per row on the byte arms, four wavefronts, incremental
    Case("sp7x100_inc_t256", RAGGED["spatial_7x100"], {"incremental_obs": True, "threads_per_env": 256}, {}, 8, 12,
         ("plane:byte/W%16", "plane2:byte/W%16", "build:inplace_stream/NW=4", "build:inplace_stream/WW=2", "cg:tables:byte/total%4")),
    # the pin kind: in place and in slots
    Case("pin40x48", RAGGED["pin_40x48"], {}, {}, 8, 12, ("build:routes=on/pin", "plane2:vector/npow2/WW1", "feat:pin/member_words>1")),
    Case("pin40x48_t256_slots", RAGGED["pin_40x48"], {"threads_per_env": 256, "num_slots": 3, "compact_features": True, "auto_reset": True}, {}, 8, 12,
         ("build:NW=4", "feat:whole/compact", "feat:CF<=NT")),
    Case("pin100x9", RAGGED["pin_100x9"], {"auto_reset": True}, {}, 8, 12, ("mask:fold/lds", "plane2:byte/W%16", "feat:rowwise/rows_cleared")),
    Case("pin100x9_slots", RAGGED["pin_100x9"], {"num_slots": 3}, {}, 8, 12, ("feat:whole/f64", "build:BUILD=slot")),
    # seven components of at most nine cells: the row-membership bit map of the pin features is one word
    Case("pin12x20_small", lambda: EnvConfig.pin(12, 20, 5, 5, 2, 3, 2, 3, 7, 3, 2, 4, 4, 2, "beam", 2, 0.5), {"auto_reset": True}, {}, 8, 9,
         ("feat:pin/member_words=1", "feat:rowwise/rows_cleared", "plane2:byte/W%16")),
    # 192 pins: the walk over the Q1 losers with np > 64, on one wavefront and on four
    Case("pin70x80_np192_t64", lambda: EnvConfig.pin(70, 80, 5, 5, 2, 6, 2, 6, 20, 10, 8, 16, 12, 2, "centroid", 2, 0.5), {"threads_per_env": 64}, {}, 6, 12,
         ("feat:pin-q1/np>64", "plane2:vector/npow2/WW2", "build:NW=1")),
    Case("pin70x80_np192_t256", lambda: EnvConfig.pin(70, 80, 5, 5, 2, 6, 2, 6, 20, 10, 8, 16, 12, 2, "centroid", 2, 0.5), {"threads_per_env": 256}, {}, 6, 12,
         ("feat:pin-q1/np>64", "build:NW=4", "build:inplace_stream/NW=4")),
    # c3 / c4: the geometry-fixed build, and its refusal by cell tensors at offset 4 and at an odd offset
    Case("c3_aligned", lambda: named_config("c3"), {}, {}, 6, 9, ("build:geo64", "plane2:vector/fixed64", "feat:pin-q1/np<=64")),
    Case("c3_off4", lambda: named_config("c3"), {}, {"grid": 4, "action_mask": 4}, 6, 9, ("build:geo64-refused/c3", "plane2:byte/misaligned", "plane:byte/misaligned")),
    Case("c3_odd", lambda: named_config("c3"), {}, {"grid": 3, "action_mask": 7}, 6, 9, ("build:geo64-refused/c3", "plane2:byte/misaligned")),
    Case("c4_aligned", lambda: named_config("c4"), {}, {}, 6, 9, ("build:geo64", "plane2:vector/fixed64", "pin_grid:out/chunks/K>=8", "cg:tables:chunks/notail")),
    Case("c4_off4", lambda: named_config("c4"), {}, {"grid": 4, "action_mask": 4, "pin_grid": 4, "component_grid": 4}, 6, 9,
         ("build:geo64-refused/c4", "pin_grid:out/byte/misaligned", "plane2:byte/misaligned", "cg:tables:chunks/notail")),
    Case("c4_odd_inc", lambda: named_config("c4"), _INC, {"grid": 5, "action_mask": 1, "pin_grid": 9, "component_grid": 3}, 6, 9,
         ("build:geo64-refused/c4", "pin_grid:out/byte/misaligned", "cg:tables:byte/misaligned")),
    Case("c4_inc", lambda: named_config("c4"), _INC, {}, 6, 9, ("plane:vector/pow2/partial", "build:geo64")),
    # rect and square: the streaming in-place builds at two words per row, and a slot build each
    Case("rect33x65", RAGGED["rect_33x65"], {"auto_reset": True}, {}, 8, 12, ("build:inplace_stream/kind=rect", "build:inplace_stream/WW=2", "plane:byte/W%16")),
    Case("rect11x96", lambda: EnvConfig.rect(11, 96, 2, 6, 2, 6, 8, 2), {}, {}, 8, 10, ("plane:vector/npow2/WW2", "build:inplace_stream/kind=rect", "feat:CF<=NT")),
    Case("rect11x96_off4_slots", lambda: EnvConfig.rect(11, 96, 2, 6, 2, 6, 8, 2), {"num_slots": 3, "compact_features": True, "auto_reset": True},
         {"grid": 4, "action_mask": 4}, 8, 10, ("plane:byte/misaligned", "feat:whole/compact")),
    Case("square3x128", RAGGED["square_3x128"], {}, {}, 8, 12, ("build:inplace_stream/kind=square", "build:inplace_stream/WW=2", "plane:vector/pow2")),
    Case("square70x12_t256", RAGGED["square_70x12"], {"threads_per_env": 256, "auto_reset": True}, {"action_mask": 3}, 8, 12,
         ("build:inplace_stream/kind=square", "build:inplace_stream/NW=4", "plane:byte/W%16")),
    Case("square3x128_slots", RAGGED["square_3x128"], {"num_slots": 3}, {"grid": 4}, 6, 8, ("build:kind=square", "build:BUILD=slot", "plane:byte/misaligned")),
)}


def call_seed(name, index):
    return zlib.crc32(f"emission:{name}:{index}".encode()) & 0x3FFFFFFF


def corrupt(actions, p_bad, seed):
    """Run.step's corruption of drawn actions: a few rows replaced by tuples that may or may not be legal."""
    a = actions.copy()
    if p_bad:
        rng = np.random.RandomState(seed)
        bad = rng.rand(len(a)) < p_bad
        a[bad] = rng.randint(-1, 70, size=(int(bad.sum()), 3))
    return a


def gather_index(B, seed):
    """A permutation with some -1."""
    rng = np.random.RandomState(seed)
    idx = rng.permutation(B).astype(np.int64)
    idx[rng.rand(B) < 0.25] = -1
    idx[0] = -1 if (idx >= 0).all() else idx[0]
    if (idx < 0).all():
        idx[1] = 0
    return idx


def _npins(rec):
    return int(np.frombuffer(np.ascontiguousarray(rec[:12]).tobytes(), np.int32)[2])


def _ncomp(rec):
    return int(np.frombuffer(np.ascontiguousarray(rec[:12]).tobytes(), np.int32)[0])


class Plan:
    """The script of a case on the CPU.  calls[j]: dict(op, seed, slot = the slot the call writes, rows = the rows it
    writes (bool [B]), and by op: actions int32 [B, 3] (as stepped), drawn (before the corruption), mask, index).
    events: what `paths` reads.  In the trajectory layout every call that writes selects the slot behind the selected
    one first, so that it meets a slot the test has dirtied."""

    def __init__(self, case, seed=None):
        if isinstance(case, str):
            case = CASES[case]
        self.case, self.cfg = case, case.cfg()
        self.seed = case.seed if seed is None else seed
        cfg, B, S = self.cfg, case.B, case.S
        auto = bool(case.kw.get("auto_reset"))
        square = cfg.kind == KIND_SQUARE
        has_info = cfg.kind in (KIND_PIN, KIND_SPATIAL)
        m = self.model = HandleModel(cfg, B, S, case.Q, auto, self.seed)
        seen = np.zeros(B, bool)          # reset at least once since the bind
        placed = np.zeros(B, np.int64)    # components placed in the current episode
        episode = np.zeros(B, np.int64)
        self.calls, self.events, t = [], [], 0

        def npins_of(i):  # of the record row i takes at its next reset
            return 0 if square else _npins(m.record(i))

        def reset_event(rows, masked):
            ev = dict(op="reset", slot=m.slot, rows=[int(i) for i in np.flatnonzero(rows)], masked=masked,
                      first={int(i): not seen[i] for i in np.flatnonzero(rows)}, npins={int(i): npins_of(int(i)) for i in np.flatnonzero(rows)})
            seen[rows] = True
            placed[rows] = 0
            episode[rows] += 1
            return ev

        self.events.append(reset_event(np.ones(B, bool), False))
        m.reset()
        for j, call in enumerate(case.script):
            op, seed_j = call[0], call_seed(case.name, j)
            if S > 1:
                m.select(m.slot + 1)
            rec = dict(op=op, seed=seed_j, slot=m.slot, t=t)
            if op in ("step", "fused"):
                drawn = rc.draws(cfg, m, self.seed, 0, t)
                a = corrupt(drawn, call[1], seed_j) if op == "step" else drawn
                if square:
                    a[:, 0] = 0
                masks = [pc.action_mask_of(m.ob.env(i)).reshape(-1, cfg.height, cfg.width) for i in range(B)]
                valid = np.array([0 <= a[i, 0] < cfg.num_orientations and 0 <= a[i, 1] < cfg.height and 0 <= a[i, 2] < cfg.width
                                  and masks[i][a[i, 0], a[i, 1], a[i, 2]] != 0 for i in range(B)])
                ncomp = np.array([0 if square else _ncomp(m.inst[i]) for i in range(B)])
                last = valid & (placed + 1 == ncomp) & (not square)
                before = [m.ob.env(i).obs()["grid"] for i in range(B)] if case.kw.get("incremental_obs") else None
                nxt = [npins_of(i) for i in range(B)] if auto else [0] * B
                rr, dd, ii = m.step(a)
                rng_rows = [(0, cfg.height)] * B
                if before is not None:
                    for i in np.flatnonzero(valid):
                        ch = np.flatnonzero((m.ob.env(int(i)).obs()["grid"] != before[i]).any(axis=1))
                        rng_rows[i] = (int(ch[0]), int(ch[-1]) + 1)
                worst = (dd != 0) & (ii[:, 0] == cfg.max_wirelength) & (ii[:, 1] == cfg.max_num_intersections) if has_info else np.zeros(B, bool)
                placed[valid] += 1
                self.events.append(dict(op="step", slot=m.slot, valid=valid.tolist(), placed_all=last.tolist(), range=rng_rows,
                                        done=(dd != 0).tolist(), npins_next=nxt, worst=worst.tolist(), episode=episode.tolist()))
                if auto:
                    d = dd != 0
                    seen[d] = True
                    placed[d] = 0
                    episode[d] += 1
                rec.update(actions=a, drawn=drawn, rows=np.ones(B, bool), reward=np.array(rr), done=np.array(dd), info=np.array(ii))
                t += 1
            elif op in ("reset_mask", "reset_done"):
                mask = rc.reset_mask(B, call[1], seed_j) if op == "reset_mask" else (m.last_done() != 0).astype(np.uint8)
                rows = mask.astype(bool)
                self.events.append(reset_event(rows, True))
                m.reset(mask)
                rec.update(mask=mask, rows=rows)
            elif op == "gather":
                idx = gather_index(B, seed_j)
                pl, ep = placed.copy(), episode.copy()
                take = m.gather(idx)
                for i in np.flatnonzero(take):
                    placed[i], episode[i] = pl[idx[i]], ep[i] + 1  # (a new episode of row i as far as its pin_grid arms go)
                seen[take] = True
                self.events.append(dict(op="gather", slot=m.slot, rows=[int(i) for i in np.flatnonzero(take)]))
                rec.update(index=idx, rows=take)
            else:
                raise KeyError(op)
            self.calls.append(rec)

    def paths(self, policy=None):
        """The labels of the plan: under one store policy, or (None) under both."""
        out = set()
        for p in ([policy] if policy else list(POLICIES)):
            out |= paths(self.cfg, self.case.layout(p), self.events)
        return out

    def instantiations(self):
        return sorted({instantiation(self.case.layout(p)) for p in POLICIES})


def pick_seed(name, seeds=SEEDS):
    """The first seed at which the plan reaches every label the case is in the table for (None: none) and what each misses."""
    missed = {}
    for s in seeds:
        got = Plan(name, seed=s).paths()
        missed[s] = [n for n in CASES[name].needs if n not in got]
        if not missed[s]:
            return s, missed
    return None, missed


@lru_cache(maxsize=None)
def plan(name):
    """The plan of a case at its seed, computed once and shared: nothing may change it."""
    return Plan(name)
