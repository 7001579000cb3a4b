"""BatchedPlacementEnv: thousands of independent placement environments on one MI355X.

The host-side mirror of the reference `gym.Env` classes
(`environment/dummy_env_{square,rectangular,rectangular_pin,rectangular_pin_spatial}.py`):
same observation keys, same action encoding, `reset()` / `step()` with a leading
batch dimension.  Observations are torch tensors that live on the device and are
updated in place by every call (the reference returns fresh copies -- `.clone()`
where copy semantics are needed).  All compute happens in libpcbenv.so's HIP
kernels on the current torch stream; nothing here touches observation data.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _frontier_lib, _frontier_sample_lib, _gumbel_leaves_lib, _gumbel_lib, _gumbel_tree_leaves_lib, _gumbel_tree_lib, _leaves_lib, _lib, _move_lib, _noise_lib, _priors_lib, _search_lib, _train_lib
from .config import EnvConfig, KIND_PIN, KIND_RECT, KIND_SPATIAL, KIND_SQUARE
from .instances import Instance, InstanceStream, env_seed, pack_instances


FEATURE_KEYS = ("all_components_feature", "placement_mask", "component_mask", "all_pins_num_feature", "all_pins_cat_feature")
COMPACT_DTYPES = {"all_components_feature": torch.int16, "placement_mask": torch.uint8, "component_mask": torch.uint8,
                  "all_pins_num_feature": torch.int8, "all_pins_cat_feature": torch.int8}


def expand_compact_features(cfg: EnvConfig, compact: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Compact feature tensors (pcbenv_compact_features: int16 / int8 / uint8) -> the reference's float64 tensors, bit
    for bit: every element is a small integer except all_components_feature[..., 4], carried as h * w and divided by
    H * W here in float64 -- the one IEEE division the reference does (`area / grid_area`, S:203-239).  The divisor is a
    tensor on the features' device: by a Python number torch divides on a GPU by multiplying with the reciprocal, which
    is one bit off for many h * w unless H * W is a power of two (9 / 448 on a 14 x 32 grid)."""
    out = {}
    for k, t in compact.items():
        f = t.to(torch.float64)
        if k == "all_components_feature":
            f[..., 4] = f[..., 4] / torch.full((), float(cfg.height * cfg.width), dtype=torch.float64, device=f.device)
        out[k] = f
    return out


def obs_spec(cfg: EnvConfig) -> Dict[str, tuple]:
    """key -> (shape without batch dim, torch dtype); keys and shapes are the reference's."""
    H, W, k = cfg.height, cfg.width, cfg.kind
    u8, f64 = torch.uint8, torch.float64
    if k == KIND_SQUARE:
        return {"grid": ((H, W), u8), "action_mask": ((H, W), u8)}
    Cc = cfg.max_num_components
    if k == KIND_RECT:
        return {"grid": ((H, W), u8), "action_mask": ((2, H, W), u8), "all_components_feature": ((Cc, 5), f64),
                "component_mask": ((Cc,), f64), "placement_mask": ((Cc,), f64)}
    mp, N = cfg.max_num_pins_per_component, cfg.max_num_nets
    if k == KIND_PIN:
        return {"grid": ((H, W), u8), "action_mask": ((4, H, W), u8), "all_components_feature": ((Cc, 5), f64),
                "placement_mask": ((Cc,), f64), "all_pins_num_feature": ((Cc, mp, 4), f64),
                "all_pins_cat_feature": ((Cc, mp, 1), f64)}
    return {"grid": ((H, W), u8), "pin_grid": ((H, W, N + 1), u8),
            "component_grid": ((Cc, cfg.max_component_h, cfg.max_component_w, N + 1), u8),
            "action_mask": ((4, H, W), u8), "all_components_feature": ((Cc, 5 + mp), f64),
            "placement_mask": ((Cc,), f64), "all_pins_num_feature": ((Cc * mp + 1, 4), f64),
            "all_pins_cat_feature": ((Cc * mp + 1, 2), f64)}


@dataclass
class Playout:
    """What `BatchedPlacementEnv.playout` returns, one row per playout (n = number of playouts)."""
    reward: torch.Tensor            # [n] float64: the reward of the last transition played (not a sum)
    done: torch.Tensor              # [n] uint8: 0 where the playout was cut at max_steps
    length: torch.Tensor            # [n] int32: transitions played
    info: Optional[torch.Tensor]    # [n, 2] float64 (wirelength, num_intersections), NaN where empty; None for square / rect
    actions: Optional[torch.Tensor] # [actions_steps, n, 3] int32, rows t >= length are zero; None if actions_steps == 0
    leaf_mask: Optional[torch.Tensor] = None  # [n, 2, H, WW] int64 like mask_bits(): the legal mask of the node each path ends in (leaf_mask=True)


def default_max_steps(cfg: EnvConfig) -> int:
    """The most transitions an episode can have: one per component (square: one per n x n tile of the grid)."""
    if cfg.kind == KIND_SQUARE:
        return (cfg.height // cfg.component_n) * (cfg.width // cfg.component_n)
    return cfg.max_num_components


class _ExternalBlock:
    """__cuda_array_interface__ view over library-owned device memory (no ownership)."""

    def __init__(self, ptr: int, nbytes: int):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def _as_tensor(ptr: int, nbytes: int, device) -> torch.Tensor:
    return torch.as_tensor(_ExternalBlock(ptr, nbytes), device=device)


LOGITS_DTYPES = (torch.float32, torch.bfloat16)


def _logits_dtype(logits) -> int:
    """The library's code (`_lib.LOGITS_*`) for a float32 or bfloat16 tensor of logits; ValueError otherwise."""
    if not isinstance(logits, torch.Tensor) or logits.dtype not in LOGITS_DTYPES:
        raise ValueError("logits must be a float32 or bfloat16 tensor")
    return _lib.LOGITS_F32 if logits.dtype == torch.float32 else _lib.LOGITS_BF16


def check_tensor(device, name, t, dtype, shape) -> None:
    """The one test of a caller's tensor before its address goes to a launch: `t` is a tensor of `dtype` (one torch dtype
    or a tuple of them) and exactly `shape`, C-contiguous -- no copy is made -- and on `device`, index included
    (`t.device == device`); ValueError naming the argument otherwise.  An entry of `shape` that is not a number ("N")
    stands for a size that could not be read off the tensors: it matches nothing."""
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    if (isinstance(t, torch.Tensor) and t.dtype in dtypes and tuple(t.shape) == tuple(shape) and t.is_contiguous()
            and t.device == device):
        return
    got = type(t).__name__ if not isinstance(t, torch.Tensor) else (
        f"{t.dtype} [{', '.join(map(str, t.shape))}] on {t.device}" + ("" if t.is_contiguous() else ", not contiguous"))
    raise ValueError(f"{name}: must have shape [{', '.join(map(str, shape))}] and dtype {' or '.join(map(str, dtypes))}, "
                     f"must be C-contiguous (no copy is made) and must be on {device}; got {got}")


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """The address of an optional tensor argument: None (a null pointer) for None."""
    return None if t is None else t.data_ptr()


def _puct_tree_want(P, N, own, slots=()):
    """dtype and shape of every tensor of a PUCT tree of P roots with N slots each (include/pcbenv_search.h), in the order
    the requests check them: the per-root tensors, `own` -- the request's own tensors, name -> (dtype, shape) -- then the
    [P, N] ones, `slots` naming further int32 ones."""
    i32, f64 = torch.int32, torch.float64
    want = {"num_nodes": (i32, (P,)), "node_action": (i32, (P, N, 3)), "terminal": (torch.uint8, (P, N)), "reward_lo": (f64, (P,)),
            "reward_hi": (f64, (P,)), **own}
    want.update({n: (i32, (P, N)) for n in ("parent", "depth", "visits", "num_children", "first_child") + tuple(slots)})
    want.update({n: (f64, (P, N)) for n in ("prior", "value_sum", "value_max")})
    return want


def _exchange_want(T, R):
    """dtype and shape of what SELECT writes for R rows: `selected`, `path_len` and `paths` of at most T levels."""
    return {"selected": (torch.int32, (R,)), "path_len": (torch.int32, (R,)), "paths": (torch.int32, (T, R, 3))}


class BatchedPlacementEnv:
    is_batched = True

    def __init__(self, cfg: EnvConfig, num_envs: int, device="cuda:0", queue_depth: int = 1,
                 run_seed: int = 0, first_env_index: int = 0, incremental_obs: bool = False,
                 auto_reset: bool = False, threads_per_env: int = 0,
                 mask_marginals: bool = False, num_slots: int = 1, options: Optional[Dict[str, int]] = None,
                 compact_features: bool = False, allocator=None):
        """num_slots > 1: trajectory layout -- every output tensor is allocated `[num_slots, B, ...]` (`self.traj`,
        `self.traj_reward`, ...), `select_slot(s)` chooses the slot the next reset / step writes and `self.obs`,
        `self.reward`, `self.done`, `self.info_raw` are views of that slot (pcbenv_bind_buffers_slots).
        options: tuning knobs of the handle, `pcbenv_set_option` (include/pcbenv.h): "stream_threshold_bytes",
        "terminal_teams", "gen_grid", "gen_lanes", "fixed_geometry" -- none changes a result.
        compact_features (trajectory layout only): the feature tensors are kept as int16 / int8 / uint8
        (`pcbenv_bind_compact_features`: 8x fewer feature bytes per step) under the same keys of `traj` / `obs`;
        `obs_f64()` / `expand_compact_features` give the reference's float64 tensors, bit for bit.
        allocator: `f(name, shape, dtype) -> device tensor` for the observation tensors (default torch.zeros); lets a
        caller place them (tools/c5_modes.py studies where the big cell tensors should sit).  The tensors may hold
        anything and need only the alignment of their element type: the first unmasked reset writes every byte of the
        selected slot (tests/test_emission_gpu.py binds sentinel-filled, misplaced views); slots no call has written
        keep what the allocator left in them."""
        cfg.validate()
        self.cfg, self.num_envs, self.queue_depth = cfg, int(num_envs), int(queue_depth)
        self.run_seed, self.first_env_index = int(run_seed), int(first_env_index)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("BatchedPlacementEnv needs a GPU device (there is no CPU fallback)")
        # the device the handle lives on, index included: one named without an index is the current device, now and for good
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self._L = _frontier_sample_lib.bind(_frontier_lib.bind(_gumbel_tree_leaves_lib.bind(_gumbel_tree_lib.bind(_gumbel_leaves_lib.bind(_gumbel_lib.bind(_noise_lib.bind(_leaves_lib.bind(_train_lib.bind(_move_lib.bind(_priors_lib.bind(_search_lib.bind(_lib.load()))))))))))))
        # per-environment spaces (the reference constructors' declarations); every tensor adds a leading batch dim
        from .spaces import action_space_for, observation_space_for
        self.action_space = self.single_action_space = action_space_for(cfg)
        self.observation_space = self.single_observation_space = observation_space_for(cfg)
        self.auto_reset = bool(auto_reset)
        self._ccfg = _lib.make_config(cfg, num_envs, queue_depth,
                                      (_lib.FLAG_INCREMENTAL_OBS if incremental_obs else 0)
                                      | (_lib.FLAG_AUTO_RESET if auto_reset else 0))
        self._ccfg.threads_per_env = int(threads_per_env)  # 0 = auto; 64 / 256 threads (1 / 4 waves) per environment
        h = C.c_void_p()
        _lib.check(self._L.pcbenv_create(C.byref(self._ccfg), self.device.index, C.byref(h)))
        self._h = h
        for name, value in (options or {}).items():
            self.set_option(name, value)
        B = self.num_envs
        S = self.num_slots = int(num_slots)
        self.compact_features = bool(compact_features)
        if self.compact_features and S < 2:
            raise ValueError("compact_features needs the trajectory layout (num_slots > 1)")
        alloc = allocator or (lambda name, shape, dtype: torch.zeros(shape, dtype=dtype, device=self.device))
        with torch.cuda.device(self.device):
            self.traj: Dict[str, torch.Tensor] = {
                k: alloc(k, (S, B) + shape, COMPACT_DTYPES[k] if self.compact_features and k in FEATURE_KEYS else dt)
                for k, (shape, dt) in obs_spec(cfg).items()}
            self.traj_reward = torch.zeros((S, B), dtype=torch.float64, device=self.device)
            self.traj_done = torch.zeros((S, B), dtype=torch.uint8, device=self.device)
            self.traj_info = torch.full((S, B, 2), float("nan"), dtype=torch.float64, device=self.device)
            self._actions = torch.zeros((B, 3), dtype=torch.int32, device=self.device)
            O = cfg.num_orientations
            # marginals of action_mask for factorised policies (not reference observation keys)
            self.traj_marginals = {"orientation": torch.zeros((S, B, O), dtype=torch.uint8, device=self.device),
                                   "rows": torch.zeros((S, B, O, cfg.height), dtype=torch.uint8, device=self.device)} if mask_marginals else {}
        bufs = _lib.PcbenvBuffers()
        for name in _lib.BUFFER_FIELDS:
            t = self.traj.get(name)
            if name == "reward":
                t = self.traj_reward
            elif name == "done":
                t = self.traj_done
            elif name == "info":
                t = self.traj_info if cfg.kind in (KIND_PIN, KIND_SPATIAL) else None
            elif name == "mask_orientation":
                t = self.traj_marginals.get("orientation")
            elif name == "mask_rows":
                t = self.traj_marginals.get("rows")
            if self.compact_features and name in FEATURE_KEYS:
                t = None  # not produced in float64: the compact twin is bound below
            setattr(bufs, name, _ptr(t))
        _lib.check(self._L.pcbenv_bind_buffers_slots(self._h, C.byref(bufs), S), self._h)
        if self.compact_features:
            cb = _lib.PcbenvCompactFeatures()
            for name in _lib.COMPACT_FIELDS:
                t = self.traj.get(name)
                setattr(cb, name, _ptr(t))
            _lib.check(self._L.pcbenv_bind_compact_features(self._h, C.byref(cb)), self._h)
        self.slot = -1
        self.select_slot(0)
        self._last_done = self.done  # `done` of the latest step (it may live in another slot than the selected one)
        self._streams: Optional[List[InstanceStream]] = None
        self._native = None
        self.device_instances = False  # True once the on-device generator owns the queue (enable_device_instances)
        torch.cuda.synchronize(self.device)

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            torch.cuda.synchronize(self.device)
            self._L.pcbenv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name: str, value: int):
        code = {"stream_threshold_bytes": _lib.OPT_STREAM_THRESHOLD_BYTES, "terminal_teams": _lib.OPT_TERMINAL_TEAMS,
                "gen_grid": _lib.OPT_GEN_GRID, "gen_lanes": _lib.OPT_GEN_LANES, "fixed_geometry": _lib.OPT_FIXED_GEOMETRY}[name]
        _lib.check(self._L.pcbenv_set_option(self._h, code, int(value)), self._h)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _log_prob_entropy(self, n: int):
        """The (log_prob, entropy) a policy call returns: float32 [n], for the kernel to fill."""
        return torch.empty(n, dtype=torch.float32, device=self.device), torch.empty(n, dtype=torch.float32, device=self.device)

    def _error_word(self, check: bool) -> Optional[torch.Tensor]:
        """The zeroed int32 [1] a kernel ORs its error bits into, for a call with check=True; None otherwise."""
        return torch.zeros(1, dtype=torch.int32, device=self.device) if check else None

    def select_slot(self, slot: int):
        """The slot of the `[num_slots, B, ...]` tensors the next reset / step writes; `obs`, `reward`, `done`,
        `info_raw`, `mask_marginals` become views of it."""
        slot = int(slot) % self.num_slots
        if slot == self.slot:
            return
        _lib.check(self._L.pcbenv_select_slot(self._h, slot), self._h)
        self.slot = slot
        self.obs: Dict[str, torch.Tensor] = {k: v[slot] for k, v in self.traj.items()}
        self.reward, self.done, self.info_raw = self.traj_reward[slot], self.traj_done[slot], self.traj_info[slot]
        self.mask_marginals = {k: v[slot] for k, v in self.traj_marginals.items()}

    def obs_f64(self, slot: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """The observation of `slot` (default: the selected one) with the feature tensors in the reference's float64
        (cell tensors stay uint8 views) -- what `obs` is without compact_features."""
        obs = self.obs if slot is None else {k: v[int(slot) % self.num_slots] for k, v in self.traj.items()}
        if not self.compact_features:
            return dict(obs)
        out = {k: v for k, v in obs.items() if k not in FEATURE_KEYS}
        out.update(expand_compact_features(self.cfg, {k: v for k, v in obs.items() if k in FEATURE_KEYS}))
        return out

    # -- instances --------------------------------------------------------------------------
    def load_instances(self, instances: Sequence[Instance], slot: int = 0, env_ids: Optional[Sequence[int]] = None):
        """Queue one instance per environment (or per listed env id) into `slot`."""
        if self.cfg.kind == KIND_SQUARE:
            return
        packed = np.ascontiguousarray(pack_instances(self.cfg, instances))
        self.load_packed(packed, slot, env_ids)

    def _host_queue_only(self, what: str):
        if self.device_instances:
            raise RuntimeError(f"{what}: the on-device generator owns the instance queue (enable_device_instances); "
                               "host-side records can no longer be queued")

    def load_packed(self, packed: np.ndarray, slot: int = 0, env_ids: Optional[Sequence[int]] = None):
        self._host_queue_only("load_instances")
        ids = None if env_ids is None else np.ascontiguousarray(env_ids, np.int32)
        _lib.check(self._L.pcbenv_load_instances(
            self._h, None if ids is None else ids.ctypes.data, packed.shape[0], slot, packed.ctypes.data,
            self._stream()), self._h)

    def generate_instances(self, native: bool = True, verify: int = 0, threads: int = 8):
        """Fill every queue slot from per-environment reference RNG streams (seed = f(run_seed, global env index)):
        slot s holds each environment's next reset instance, exactly what the reference env seeded with that
        stream seed would draw at that `reset()`.  `native=True` uses libpcbenv.so's generator
        (csrc/instance_gen.cpp, ~100x faster); `native=False` the NumPy/`random`-calling `InstanceStream`;
        `verify=n` cross-checks the first n environments of every slot between the two.
        Returns the packed records per slot (uint8 [B, instance_stride])."""
        if self.cfg.kind == KIND_SQUARE:
            return []
        self._host_queue_only("generate_instances")
        mode = ("native", bool(verify)) if native else ("numpy", False)
        if getattr(self, "_gen_mode", mode) != mode:
            raise RuntimeError("generate_instances: keep the same generator (native / verify) for the lifetime of the "
                               "environment -- every call continues the per-environment RNG streams")
        self._gen_mode = mode
        seeds = [env_seed(self.run_seed, self.first_env_index + i) for i in range(self.num_envs)]
        if native and self._native is None:
            from .instances import NativeInstanceStreams
            self._native = NativeInstanceStreams(self.cfg, seeds, threads)
        if (not native or verify) and self._streams is None:
            n = self.num_envs if not native else min(verify, self.num_envs)
            self._streams = [InstanceStream(self.cfg, seeds[i]) for i in range(n)]
        out = []
        for s in range(self.queue_depth):
            if native:
                packed = self._native.next_packed()
                if verify:
                    ref = pack_instances(self.cfg, [st.next() for st in self._streams])
                    if not np.array_equal(packed[:len(ref)], ref):
                        raise RuntimeError("native instance generator disagrees with InstanceStream")
            else:
                packed = np.ascontiguousarray(pack_instances(self.cfg, [st.next() for st in self._streams]))
            self.load_packed(packed, slot=s)
            out.append(packed)
        return out

    def enable_device_instances(self):
        """Fresh instances at every reset, generated on the device (csrc/pcb_geninst.h): environment i draws stream
        `env_seed(run_seed, first_env_index + i)`, the same records `generate_instances()` would queue, episode after
        episode, without the host in the loop.  The library owns the queue from here on."""
        if self.cfg.kind == KIND_SQUARE:
            return
        seeds = np.asarray([env_seed(self.run_seed, self.first_env_index + i) for i in range(self.num_envs)], np.int64)
        if seeds.min() < 0 or seeds.max() >= 2 ** 32:
            raise ValueError("stream seeds must fit 32 bits (np.random.seed)")
        s32 = np.ascontiguousarray(seeds, np.uint32)
        _lib.check(self._L.pcbenv_instgen_device_enable(self._h, s32.ctypes.data, self._stream()), self._h)
        self.device_instances = True

    def device_instance_errors(self) -> int:
        err = C.c_uint32()
        _lib.check(self._L.pcbenv_instgen_device_status(self._h, C.byref(err), self._stream()), self._h)
        return int(err.value)

    def queued_instances(self, slot: int) -> np.ndarray:
        """Packed records of one queue slot, uint8 [B, instance_stride] (synchronises)."""
        from .instances import instance_stride
        out = np.zeros((self.num_envs, instance_stride(self.cfg)), np.uint8)
        _lib.check(self._L.pcbenv_get_instances(self._h, int(slot), out.ctypes.data, self._stream()), self._h)
        return out

    def refill_slot(self, slot: int, native: bool = True):
        """Overwrite one queue slot with every environment's next instance (call when no environment can be
        about to read that slot, e.g. between rollouts; copies are ordered on the current stream)."""
        if self.cfg.kind == KIND_SQUARE:
            return None
        self._host_queue_only("refill_slot")
        if native:
            if self._native is None:
                raise RuntimeError("call generate_instances(native=True) first")
            packed = self._native.next_packed()
        else:
            packed = np.ascontiguousarray(pack_instances(self.cfg, [st.next() for st in self._streams]))
        self.load_packed(packed, slot=slot)
        return packed

    # -- gym-style API ----------------------------------------------------------------------
    def reset(self, mask: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        m = None
        if mask is not None:
            m = mask.to(device=self.device, dtype=torch.uint8).contiguous()
        _lib.check(self._L.pcbenv_reset(self._h, None if m is None else m.data_ptr(), self._stream()), self._h)
        return self.obs

    def reset_done(self) -> Dict[str, torch.Tensor]:
        """Explicit auto-reset: environments whose last step returned done take their next instance."""
        _lib.check(self._L.pcbenv_reset(self._h, self._last_done.data_ptr(), self._stream()), self._h)
        return self.obs

    def step(self, actions: torch.Tensor):
        """actions: int tensor [B, 3] = (orientation, x, y) ([B, 2] = (x, y) for the square env) or flat [B]
        (`a = o*H*W + x*W + y`, utils/environment/env_wrappers.py:80-98)."""
        a = actions.to(device=self.device, dtype=torch.int32)
        if a.dim() == 1:
            fmt = _lib.ACTION_FLAT
            a = a.contiguous()
        else:
            fmt = _lib.ACTION_TUPLE
            if a.shape[1] == 2:
                self._actions[:, 1:] = a
                a = self._actions
            a = a.contiguous()
        assert a.shape[0] == self.num_envs
        _lib.check(self._L.pcbenv_step(self._h, a.data_ptr(), fmt, self._stream()), self._h)
        self._last_done = self.done
        return self.obs, self.reward, self.done, self.info

    @property
    def info(self) -> Dict[str, torch.Tensor]:
        """`wirelength` / `num_intersections` per environment; NaN where the reference's info dict is `{}`."""
        if self.cfg.kind not in (KIND_PIN, KIND_SPATIAL):
            return {}
        return {"wirelength": self.info_raw[:, 0], "num_intersections": self.info_raw[:, 1]}

    def sample_actions(self, step_index: int, flat: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Uniform draw over the legal actions of every environment, on device (random-policy counterpart).
        out: int32 [B, 3] or [B] (flat), C-contiguous, on `self.device`; not checked."""
        if out is None:
            out = torch.empty((self.num_envs,) if flat else (self.num_envs, 3), dtype=torch.int32, device=self.device)
        _lib.check(self._L.pcbenv_sample_actions(
            self._h, out.data_ptr(), _lib.ACTION_FLAT if flat else _lib.ACTION_TUPLE, self.run_seed,
            self.first_env_index, int(step_index), self._stream()), self._h)
        return out

    def sample_logits(self, logits: torch.Tensor, step_index: int, greedy: bool = False, flat: bool = False,
                      out: Optional[torch.Tensor] = None, check: bool = False):
        """A policy's masked categorical draw on the device (`pcbenv_sample_logits`, one kernel launch): the reference
        models' `logits += max(log(action_mask), float32.min)` followed by RLlib's Categorical `sample()` (or
        `deterministic_sample()` with greedy=True), `logp` and `entropy`.  logits: float32 or bfloat16 `[B, A]` or
        `[B, O, H, W]` (A = O*H*W in the flat action order), C-contiguous, on `self.device`; illegal entries are never
        read (raw or already-masked logits give identical results).  The legal set is the current `action_mask`.  The
        draw uses `run_seed` and `first_env_index` as `sample_actions` does; constant logits draw exactly what
        `sample_actions(step_index)` draws.  Returns (actions int32 [B, 3] or [B] (flat), log_prob float32 [B],
        entropy float32 [B]).  check=True synchronises and raises if a legal logit was NaN / +inf or every legal logit
        -inf (those environments then took the uniform draw)."""
        cfg, B = self.cfg, self.num_envs
        dtype = _logits_dtype(logits)
        grid = (B, cfg.num_orientations, cfg.height, cfg.width)
        check_tensor(self.device, "logits", logits, LOGITS_DTYPES, grid if logits.dim() == 4 else (B, grid[1] * grid[2] * grid[3]))
        if out is None:
            out = torch.empty((B,) if flat else (B, 3), dtype=torch.int32, device=self.device)
        check_tensor(self.device, "out", out, torch.int32, (B,) if flat else (B, 3))
        (log_prob, entropy), err = self._log_prob_entropy(B), self._error_word(check)
        _lib.check(self._L.pcbenv_sample_logits(
            self._h, logits.data_ptr(), dtype, _lib.DRAW_GREEDY if greedy else _lib.DRAW_SAMPLE, out.data_ptr(),
            _lib.ACTION_FLAT if flat else _lib.ACTION_TUPLE, log_prob.data_ptr(), entropy.data_ptr(), _ptr(err), self.run_seed,
            self.first_env_index, int(step_index), self._stream()), self._h)
        if check:
            bits = int(err.item())
            if bits:
                raise FloatingPointError(f"sample_logits: error bits {bits:#x} (1: a legal logit was NaN or +inf, 2: every "
                                         "legal logit was -inf); those environments took the uniform draw")
        return out, log_prob, entropy

    def _check_rows(self, n, logits, actions, mask_bits=None, flat_ok=False, rows=None):
        """The tensors every policy call but sample_logits takes -- logits [N, n] float32 or bfloat16, actions int32 [N, 3]
        (with flat_ok also [N]) and, where the call reads stored legal sets, mask_bits int64 [N, 2, H, WW] -> (N, the
        logits' dtype code).  N is `rows` or, without it, what logits has."""
        dtype = _logits_dtype(logits)
        N = rows if rows is not None else logits.shape[0] if logits.dim() == 2 else "N"
        check_tensor(self.device, "logits", logits, LOGITS_DTYPES, (N, n))
        check_tensor(self.device, "actions", actions, torch.int32, (N,) if flat_ok and actions.dim() == 1 else (N, 3))
        if mask_bits is not None:
            check_tensor(self.device, "mask_bits", mask_bits, torch.int64, (N, 2, self.cfg.height, (self.cfg.width + 63) // 64))
        return N, dtype

    def _check_gradient_args(self, logits, out, optional):
        """The backward calls' own tensors: `out` like logits (a fresh one for None; returned) and the float32 ones that
        may be None, (name, tensor, shape) each."""
        for name, t, shape in optional:
            if t is not None:
                check_tensor(self.device, name, t, torch.float32, shape)
        if out is None:
            return torch.empty_like(logits)
        check_tensor(self.device, "out must match logits", out, logits.dtype, logits.shape)
        return out

    def evaluate_logits_forward(self, logits, mask_bits, actions, stats: Optional[torch.Tensor] = None,
                                errors: Optional[torch.Tensor] = None):
        """`pcbenv_evaluate_logits`, one kernel launch: (log_prob, entropy) float32 [N] of the stored `actions` under the
        masked categorical of `logits` [N, A] with the legal sets `mask_bits` [N, 2, H, WW] (what `mask_bits()` returned
        when the rows were stored).  stats: float32 [N, 4] the backward call needs, or None.  errors: int32 [1] the error
        bits are ORed into, or None."""
        N, dtype = self._check_rows(self.cfg.num_orientations * self.cfg.height * self.cfg.width, logits, actions, mask_bits, flat_ok=True)
        flat = actions.dim() == 1
        if stats is not None:
            check_tensor(self.device, "stats", stats, torch.float32, (N, 4))
        log_prob, entropy = self._log_prob_entropy(N)
        if N == 0:  # torch gives empty tensors a null pointer
            return log_prob, entropy
        _lib.check(self._L.pcbenv_evaluate_logits(
            self._h, logits.data_ptr(), dtype, mask_bits.data_ptr(), actions.data_ptr(), _lib.ACTION_FLAT if flat else _lib.ACTION_TUPLE, N,
            log_prob.data_ptr(), entropy.data_ptr(), _ptr(stats), _ptr(errors), self._stream()), self._h)
        return log_prob, entropy

    def evaluate_logits_backward(self, logits, mask_bits, actions, stats, grad_log_prob, grad_entropy,
                                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`pcbenv_evaluate_logits_backward`, one kernel launch: the gradient with respect to `logits`, every element
        written (into `out`, or a fresh `torch.empty_like(logits)`).  grad_log_prob / grad_entropy: float32 [N] or None
        (zero)."""
        N, dtype = self._check_rows(self.cfg.num_orientations * self.cfg.height * self.cfg.width, logits, actions, mask_bits, flat_ok=True)
        flat = actions.dim() == 1
        out = self._check_gradient_args(logits, out, (("stats", stats, (N, 4)), ("grad_log_prob", grad_log_prob, (N,)), ("grad_entropy", grad_entropy, (N,))))
        if N == 0:
            return out
        _lib.check(self._L.pcbenv_evaluate_logits_backward(
            self._h, logits.data_ptr(), dtype, mask_bits.data_ptr(), actions.data_ptr(), _lib.ACTION_FLAT if flat else _lib.ACTION_TUPLE, N,
            _ptr(stats), _ptr(grad_log_prob), _ptr(grad_entropy), out.data_ptr(), self._stream()), self._h)
        return out

    @torch.no_grad()
    def evaluate_logits(self, logits, mask_bits, actions, errors: Optional[torch.Tensor] = None):
        """Log-probability and entropy of stored actions under the masked categorical of `logits` (the reference's
        RLlib `Categorical.logp` / `entropy` of the masked logits), without a gradient: `(log_prob, entropy)` float32
        [N].  N is arbitrary (a minibatch of stored steps).  `pcbenv.masked_categorical.evaluate` is the differentiable
        form."""
        return self.evaluate_logits_forward(logits, mask_bits, actions, None, errors)

    # -- the AlphaZero policy loss: a masked policy against the visit counts of a searched move -------------------
    def _visits_request(self, logits, mask_bits, visits, target_actions):
        """The request both visit calls start from (include/pcbenv_train.h), its four inputs checked: logits [N, A]
        float32 or bfloat16, mask_bits int64 [N, 2, H, WW], visits int32 [N, C], target_actions int32 [N, C, 3] or
        [N, C] (flat) -> (N, request)."""
        cfg = self.cfg
        dtype = _logits_dtype(logits)
        N = logits.shape[0] if logits.dim() == 2 else "N"
        Cn = visits.shape[1] if isinstance(visits, torch.Tensor) and visits.dim() == 2 else "C"
        check_tensor(self.device, "logits", logits, LOGITS_DTYPES, (N, cfg.num_orientations * cfg.height * cfg.width))
        check_tensor(self.device, "mask_bits", mask_bits, torch.int64, (N, 2, cfg.height, (cfg.width + 63) // 64))
        check_tensor(self.device, "visits", visits, torch.int32, (N, Cn))
        flat = isinstance(target_actions, torch.Tensor) and target_actions.dim() == 2
        check_tensor(self.device, "target_actions", target_actions, torch.int32, (N, Cn) if flat else (N, Cn, 3))
        R = _train_lib.PcbenvVisitsRequest
        req = R(struct_size=C.sizeof(R), logits_dtype=dtype, action_format=_lib.ACTION_FLAT if flat else _lib.ACTION_TUPLE, num_targets=Cn,
                num_rows=N, reserved=0, logits=logits.data_ptr(), mask_bits=mask_bits.data_ptr(), visits=visits.data_ptr(),
                target_actions=target_actions.data_ptr(), stream=self._stream().value)
        return N, req

    def evaluate_visits_forward(self, logits, mask_bits, visits, target_actions, stats: Optional[torch.Tensor] = None,
                                errors: Optional[torch.Tensor] = None, out: Optional[Sequence[torch.Tensor]] = None):
        """`pcbenv_evaluate_visits`, one kernel launch: (cross_entropy, entropy) float32 [N] of the masked categorical of
        `logits` [N, A] with the legal sets `mask_bits` [N, 2, H, WW] against the visit distribution of `visits` int32
        [N, C] over `target_actions` int32 [N, C, 3] or [N, C] (flat) -- what `puct_move` CHOOSE wrote as child_visits /
        child_actions.  stats: float32 [N, 4] the backward call needs, or None.  errors: int32 [1] the error bits are ORed
        into (1: a legal NaN or +inf, 2: every legal logit -inf, 4: an entry with negative visits or a visited action
        that is out of range or not legal), or None.  out: two float32 [N] tensors to write into."""
        N, req = self._visits_request(logits, mask_bits, visits, target_actions)
        if stats is not None:
            check_tensor(self.device, "stats", stats, torch.float32, (N, 4))
        if errors is not None:
            check_tensor(self.device, "errors", errors, torch.int32, (1,))
        cross_entropy, entropy = self._log_prob_entropy(N) if out is None else out
        check_tensor(self.device, "out[0] (cross_entropy)", cross_entropy, torch.float32, (N,))
        check_tensor(self.device, "out[1] (entropy)", entropy, torch.float32, (N,))
        if N == 0:  # torch gives empty tensors a null pointer
            return cross_entropy, entropy
        req.cross_entropy, req.entropy, req.stats, req.errors_dev = cross_entropy.data_ptr(), entropy.data_ptr(), _ptr(stats), _ptr(errors)
        _lib.check(self._L.pcbenv_evaluate_visits(self._h, C.byref(req)), self._h)
        return cross_entropy, entropy

    def evaluate_visits_backward(self, logits, mask_bits, visits, target_actions, stats, grad_cross_entropy, grad_entropy,
                                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`pcbenv_evaluate_visits_backward`, one kernel launch: the gradient with respect to `logits`, every element
        written once (into `out`, or a fresh `torch.empty_like(logits)`).  stats: what the forward call wrote for these
        rows.  grad_cross_entropy / grad_entropy: float32 [N] or None (zero)."""
        N, req = self._visits_request(logits, mask_bits, visits, target_actions)
        out = self._check_gradient_args(logits, out, (("stats", stats, (N, 4)), ("grad_cross_entropy", grad_cross_entropy, (N,)),
                                                      ("grad_entropy", grad_entropy, (N,))))
        if N == 0:
            return out
        req.stats, req.grad_cross_entropy, req.grad_entropy, req.grad_logits = _ptr(stats), _ptr(grad_cross_entropy), _ptr(grad_entropy), out.data_ptr()
        _lib.check(self._L.pcbenv_evaluate_visits_backward(self._h, C.byref(req)), self._h)
        return out

    # -- factorised policies: one action coordinate at a time ---------------------------------------------------
    def _axis_stage(self, axis, given):
        """(axis, given) of a stage -> (axis code, `given` bit set, n); `given` is a bit set or a sequence of axes."""
        axis = int(axis)
        if axis not in (_lib.AXIS_ORIENTATION, _lib.AXIS_X, _lib.AXIS_Y):
            raise ValueError(f"axis must be 0 (orientation), 1 (x) or 2 (y), got {axis}")
        bits = int(given) if isinstance(given, int) else sum({1 << int(a) for a in given})
        if bits & ~7 or bits & (1 << axis):
            raise ValueError(f"given must name axes 0..2 other than the stage's own ({axis}), got {given}")
        return axis, bits, (self.cfg.num_orientations, self.cfg.height, self.cfg.width)[axis]

    def sample_axis(self, axis, logits: torch.Tensor, step_index: int, actions: torch.Tensor, given=(),
                    greedy: bool = False, check: bool = False):
        """One stage of a factorised policy on the device (`pcbenv_sample_axis`, one kernel launch): the masked
        categorical over ONE action coordinate -- axis 0 orientation, 1 x, 2 y -- given the coordinates named in `given`
        (a sequence of axes, or the bit set), which are read from `actions` int32 [B, 3]; the drawn value is written into
        column `axis` of `actions` and the remaining column is left alone.  logits: float32 or bfloat16 [B, n] with
        n = O, H or W, C-contiguous; entries outside the stage's legal set are never read.  The legal set comes from the
        current state's bit rows (the reference's reduce_max / gather of `action_mask`,
        utils/agent/factorized_action_distributions.py:107-818).  Returns (log_prob, entropy) float32 [B].  check=True
        synchronises and raises if a logit of a legal set was NaN / +inf, every one -inf, or a given value out of range."""
        axis, bits, n = self._axis_stage(axis, given)
        N, dtype = self._check_rows(n, logits, actions, rows=self.num_envs)  # the sampler's rows are the handle's environments
        (log_prob, entropy), err = self._log_prob_entropy(N), self._error_word(check)
        _lib.check(self._L.pcbenv_sample_axis(
            self._h, axis, bits, logits.data_ptr(), dtype, _lib.DRAW_GREEDY if greedy else _lib.DRAW_SAMPLE,
            actions.data_ptr(), log_prob.data_ptr(), entropy.data_ptr(), _ptr(err),
            self.run_seed, self.first_env_index, int(step_index), self._stream()), self._h)
        if check:
            e = int(err.item())
            if e:
                raise FloatingPointError(f"sample_axis: error bits {e:#x} (1: a logit of a legal set was NaN or +inf, 2: every "
                                         "one was -inf -- those rows took the uniform pick; 8: a given value out of range)")
        return log_prob, entropy

    def evaluate_axis_forward(self, axis, given, logits, mask_bits, actions, errors: Optional[torch.Tensor] = None):
        """`pcbenv_evaluate_axis`, one kernel launch: (log_prob, entropy) float32 [N] of the values stored in column
        `axis` of `actions` int32 [N, 3] under the stage's masked categorical of `logits` [N, n], with the legal sets
        derived from `mask_bits` int64 [N, 2, H, WW] and the given columns of `actions`.  errors: int32 [1] the error bits
        are ORed into, or None."""
        axis, bits, n = self._axis_stage(axis, given)
        N, dtype = self._check_rows(n, logits, actions, mask_bits)
        log_prob, entropy = self._log_prob_entropy(N)
        if N == 0:  # torch gives empty tensors a null pointer
            return log_prob, entropy
        _lib.check(self._L.pcbenv_evaluate_axis(
            self._h, axis, bits, logits.data_ptr(), dtype, mask_bits.data_ptr(), actions.data_ptr(), N, log_prob.data_ptr(),
            entropy.data_ptr(), _ptr(errors), self._stream()), self._h)
        return log_prob, entropy

    def evaluate_axis_backward(self, axis, given, logits, mask_bits, actions, grad_log_prob, grad_entropy,
                               out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`pcbenv_evaluate_axis_backward`, one kernel launch: the gradient with respect to `logits`, every element written
        (into `out`, or a fresh `torch.empty_like(logits)`).  grad_log_prob / grad_entropy: float32 [N] or None (zero)."""
        axis, bits, n = self._axis_stage(axis, given)
        N, dtype = self._check_rows(n, logits, actions, mask_bits)
        out = self._check_gradient_args(logits, out, (("grad_log_prob", grad_log_prob, (N,)), ("grad_entropy", grad_entropy, (N,))))
        if N == 0:
            return out
        _lib.check(self._L.pcbenv_evaluate_axis_backward(
            self._h, axis, bits, logits.data_ptr(), dtype, mask_bits.data_ptr(), actions.data_ptr(), N,
            _ptr(grad_log_prob), _ptr(grad_entropy), out.data_ptr(), self._stream()), self._h)
        return out

    def rollout_step(self, step_index: int, flat: bool = False, out: Optional[torch.Tensor] = None):
        """`sample_actions` + `step` in one kernel launch (the body of the reference's random-policy
        `simulate()` loop, agent/random/random_policy_square.py:38-56); `out` receives the actions taken: int32 [B, 3] or
        [B] (flat), C-contiguous, on `self.device`; not checked."""
        if out is None:
            out = torch.empty((self.num_envs,) if flat else (self.num_envs, 3), dtype=torch.int32, device=self.device)
        _lib.check(self._L.pcbenv_step_sampled(
            self._h, out.data_ptr(), _lib.ACTION_FLAT if flat else _lib.ACTION_TUPLE, self.run_seed,
            self.first_env_index, int(step_index), self._stream()), self._h)
        self._last_done = self.done
        return self.obs, self.reward, self.done, self.info, out

    def rollout_steps(self, step_index0: int, num_steps: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`num_steps` sample+step transitions in one persistent kernel launch (use with auto_reset=True): step t
        writes slot `(self.slot + t) % num_slots`; returns the actions taken, int32 [num_steps, B, 3].  The selected
        slot is left where it was -- `select_slot(self.slot + num_steps)` continues behind the rollout.
        out: int32 [num_steps, B, 3], C-contiguous, on `self.device`; not checked."""
        if out is None:
            out = torch.empty((num_steps, self.num_envs, 3), dtype=torch.int32, device=self.device)
        _lib.check(self._L.pcbenv_rollout_sampled(
            self._h, out.data_ptr(), _lib.ACTION_TUPLE, int(num_steps), self.run_seed, self.first_env_index,
            int(step_index0), self._stream()), self._h)
        return out

    def gather_(self, index: torch.Tensor, source: Optional["BatchedPlacementEnv"] = None, check: bool = False,
                paths: Optional[torch.Tensor] = None, path_len: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """Fork / reorder episodes on the device (`pcbenv_gather`, one kernel launch, no host round trip): environment i
        continues the episode in progress of environment `index[i]` of `source` (default: this environment batch; any
        permutation or repetition), `-1` keeps i's own episode.  `source` needs an equal definition (the same EnvConfig;
        num_envs, queue_depth, flags may differ) on the same device.  Every observation tensor, reward, done and info row of i
        (selected slot) then equals what `index[i]` showed, and later steps of i go as those of `index[i]` would have.  The
        instance stream stays i's own: its next reset takes its own next instance (the one difference from
        `copy.deepcopy` of a reference env).  check=True raises IndexError if an index was out of range (such rows keep
        their episode); it synchronises the host, so it is off by default.

        Tree nodes named by a path (`pcbenv_gather_paths`, still one kernel launch; taken when `paths` or `path_len` is
        given): paths, int32 [D, B, 3] or flat [D, B], step-major like `playout(paths=...)`: after the fork, environment i
        alone makes transitions t < path_len[i] with action paths[t, i], as `step` would on a batch with auto_reset=False,
        and stops behind the first one that reports done.  The observations show the state after the last transition
        applied; reward / done / info are that transition's (with none applied: the forked row's).  A bad path action
        ends the row's path there with the worst-case reward, as `step` would.  It never resets.  path_len: int32 [B],
        default D for every row; a value outside [0, D] keeps the row's episode like a bad index (check=True raises on it
        too).  The number of transitions applied to every row is left in `self.gather_length`, int32 [B] on the device
        (0 for rows that kept their episode); without `paths` / `path_len` that attribute is left as it was."""
        src = self if source is None else source
        idx = index.to(device=self.device, dtype=torch.int32).contiguous()
        if tuple(idx.shape) != (self.num_envs,):
            raise ValueError(f"index must have shape [{self.num_envs}], got {tuple(idx.shape)}")
        use_paths = paths is not None or path_len is not None
        pa, pl, D, fmt = self._path_args(paths, path_len, self.num_envs)
        err = self._error_word(check)
        # reset_done() reads _last_done: the kernel carries `done` of the selected slots over; where _last_done lives in
        # another slot (either side), the forked rows' flags are taken from the source's _last_done here, before the
        # launch -- for the rows without a transition; those with one take the `done` the kernel wrote
        in_slot = (self._last_done.data_ptr() == self.done.data_ptr() and src._last_done.data_ptr() == src.done.data_ptr())
        if not in_slot:
            taken = (idx >= 0) & (idx < src.num_envs)
            if pl is not None:
                taken &= (pl >= 0) & (pl <= D)
            forked = src._last_done[idx.long().clamp(0, src.num_envs - 1)]
        if use_paths:
            length = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
            req = _lib.PcbenvGatherPathsRequest(
                struct_size=C.sizeof(_lib.PcbenvGatherPathsRequest), action_format=fmt, src=None if src is self else src._h,
                src_index_dev=idx.data_ptr(), path_actions_dev=_ptr(pa) if D > 0 else None, path_len_dev=_ptr(pl), path_steps=D,
                length_dev=length.data_ptr(), errors_dev=_ptr(err), stream=self._stream().value)
            _lib.check(self._L.pcbenv_gather_paths(self._h, C.byref(req)), self._h)
            self.gather_length = length
        else:
            _lib.check(self._L.pcbenv_gather(self._h, None if src is self else src._h, idx.data_ptr(), _ptr(err), self._stream()), self._h)
        if not in_slot:
            kept = torch.where(taken, forked, self._last_done)
            self._last_done = torch.where(length > 0, self.done, kept) if use_paths else kept
        bits = int(err.item()) if check else 0
        if bits and use_paths:
            raise IndexError(f"gather_: an index is outside [-1, {src.num_envs}) or a path_len outside [0, {D}] "
                             f"(error bits {bits}; those environments kept their episode)")
        if bits:
            raise IndexError(f"gather_: an index is outside [-1, {src.num_envs}) (those environments kept their episode)")
        return self.obs

    def _path_args(self, paths, path_len, n):
        """The `paths` / `path_len` of `gather_` and `playout` for n rows -> (paths, path_len, D, action format), the
        tensors int32, contiguous, on this device or None; without `paths`, D = 0 and the format is the tuple one."""
        pa, pl, D, fmt = None, None, 0, _lib.ACTION_TUPLE
        if paths is not None:
            pa = paths.to(device=self.device, dtype=torch.int32).contiguous()
            if pa.dim() not in (2, 3) or pa.shape[1] != n or (pa.dim() == 3 and pa.shape[2] != 3):
                raise ValueError(f"paths must have shape [D, {n}] (flat) or [D, {n}, 3], got {tuple(pa.shape)}")
            D = pa.shape[0]
            if pa.dim() == 2:
                fmt = _lib.ACTION_FLAT
        if path_len is not None:
            pl = path_len.to(device=self.device, dtype=torch.int32).contiguous()
            if tuple(pl.shape) != (n,):
                raise ValueError(f"path_len must have shape [{n}], got {tuple(pl.shape)}")
        return pa, pl, D, fmt

    def playout(self, k: Optional[int] = None, index: Optional[torch.Tensor] = None, step_index: int = 0,
                first_actions: Optional[torch.Tensor] = None, max_steps: Optional[int] = None,
                actions_steps: Optional[int] = None, first_env_index: int = 0, check: bool = False,
                paths: Optional[torch.Tensor] = None, path_len: Optional[torch.Tensor] = None, leaf_mask: bool = False) -> Playout:
        """Play forked episodes to their end on the device without observations (`pcbenv_playout`, one kernel launch, no
        second handle): playout i starts from the episode in progress of environment `index[i]` -- or, with `k`,
        environment i // k (k playouts per environment) -- and takes uniformly drawn legal actions until its first
        `done` or `max_steps` transitions (default: the most an episode can have).  Transition t draws what
        `rollout_step(step_index + t)` draws for environment i of a handle with `first_env_index`, this handle's
        `run_seed` and auto_reset=False after `gather_` had forked the roots into it, and the transition is that
        handle's, bit for bit.  first_actions: int32 [n, 3] or flat [n]: the action of transition 0 instead of a draw (an
        illegal one ends the playout with the worst-case reward, as `step` would).  actions_steps (default max_steps):
        how many leading actions to record.  Nothing of this environment batch changes.  check=True synchronises and
        raises IndexError if an index was out of range (those rows report length 0).

        Playouts from tree nodes (`pcbenv_playout_paths`, taken when any of the next three is given): paths, int32
        [D, n, 3] or flat [D, n], step-major like `actions`: transition t < path_len[i] of playout i applies paths[t, i]
        instead of a draw, the later ones draw as above (the draw's key depends on t, not on the path, and max_steps counts
        the path's transitions too).  path_len: int32 [n], default D for every playout; check=True also raises on a value
        outside [0, D].  A bad path action ends the playout there with the worst-case reward.  leaf_mask=True: the result's
        `leaf_mask` is the legal mask of the node each path ends in -- or of the state the episode ended in, if it ended
        on the path -- int64 [n, 2, H, WW] like `mask_bits()`, usable as the mask_bits of the evaluate calls.  `actions`
        records a path action as given.  first_actions cannot be combined with any of the three (it is a path of one step)."""
        if (k is None) == (index is None):
            raise ValueError("playout: give either k (playouts per environment) or index (the root of every playout)")
        idx = None
        if index is not None:
            idx = index.to(device=self.device, dtype=torch.int32).contiguous()
            if idx.dim() != 1:
                raise ValueError(f"index must be one-dimensional, got {tuple(idx.shape)}")
            n = idx.shape[0]
        else:
            if int(k) < 1:
                raise ValueError("k must be at least 1")
            n = self.num_envs * int(k)
        T = default_max_steps(self.cfg) if max_steps is None else int(max_steps)
        A = T if actions_steps is None else int(actions_steps)
        use_paths = paths is not None or path_len is not None or leaf_mask
        if first_actions is not None and use_paths:
            raise ValueError("playout: first_actions cannot be combined with paths, path_len or leaf_mask (give it as a path of one step)")
        fa = None
        pa, pl, D, fmt = self._path_args(paths, path_len, n)
        if D > T:
            raise ValueError(f"paths has {D} steps, max_steps is {T}")
        if first_actions is not None:
            fa = first_actions.to(device=self.device, dtype=torch.int32).contiguous()
            if tuple(fa.shape) not in ((n,), (n, 3)):
                raise ValueError(f"first_actions must have shape [{n}] (flat) or [{n}, 3], got {tuple(fa.shape)}")
            if fa.dim() == 1:
                fmt = _lib.ACTION_FLAT
        pins = self.cfg.kind in (KIND_PIN, KIND_SPATIAL)
        dev = self.device
        reward = torch.empty(n, dtype=torch.float64, device=dev)
        done = torch.empty(n, dtype=torch.uint8, device=dev)
        length = torch.empty(n, dtype=torch.int32, device=dev)
        info = torch.empty((n, 2), dtype=torch.float64, device=dev) if pins else None
        actions = torch.zeros((A, n) if fmt == _lib.ACTION_FLAT else (A, n, 3), dtype=torch.int32, device=dev) if A > 0 else None
        err = self._error_word(check)
        H, WW = self.cfg.height, (self.cfg.width + 63) // 64
        leaf = torch.empty((n, 2, H, WW), dtype=torch.int64, device=dev) if leaf_mask else None
        if n == 0:  # torch gives empty tensors a null pointer
            return Playout(reward, done, length, info, actions, leaf)
        if use_paths:
            req = _lib.PcbenvPlayoutRequest(
                struct_size=C.sizeof(_lib.PcbenvPlayoutRequest), action_format=fmt, root_index_dev=_ptr(idx), num_playouts=n,
                path_actions_dev=_ptr(pa) if D > 0 else None, path_len_dev=_ptr(pl), path_steps=D, max_steps=T, reward_dev=reward.data_ptr(),
                done_dev=done.data_ptr(), length_dev=length.data_ptr(), info_dev=_ptr(info), actions_out_dev=_ptr(actions), actions_steps=A,
                leaf_mask_bits_dev=_ptr(leaf), errors_dev=_ptr(err), seed=self.run_seed, first_env_index=int(first_env_index),
                step_index0=int(step_index), stream=self._stream().value)
            _lib.check(self._L.pcbenv_playout_paths(self._h, C.byref(req)), self._h)
            if check and int(err.item()) != 0:
                raise IndexError(f"playout: an index is outside [0, {self.num_envs}) or a path_len outside [0, {D}] (those playouts report length 0)")
            return Playout(reward, done, length, info, actions, leaf)
        _lib.check(self._L.pcbenv_playout(
            self._h, _ptr(idx), n, _ptr(fa), fmt, T, reward.data_ptr(), done.data_ptr(), length.data_ptr(), _ptr(info),
            _ptr(actions), A, _ptr(err), self.run_seed, int(first_env_index), int(step_index), self._stream()), self._h)
        if check and int(err.item()) != 0:
            raise IndexError(f"playout: an index is outside [0, {self.num_envs}) (those playouts report length 0)")
        return Playout(reward, done, length, info, actions)

    def _tree_request(self, Request, tree, want, **scalars):
        """A `Request` with `scalars` and the address of every tensor `want` names (name -> (dtype, shape)) taken from `tree`
        after `check_tensor`; `errors_dev` is optional."""
        if tree.get("errors_dev") is not None:
            want["errors_dev"] = (torch.int32, (1,))
        req = Request(struct_size=C.sizeof(Request), **scalars)
        for name, (dtype, shape) in want.items():
            check_tensor(self.device, name, tree[name], dtype, shape)
            setattr(req, name, _ptr(tree[name]))
        return req

    def _advance(self, call, req, phases, inputs) -> None:
        """One launch of a tree entry point: `phases` and the optional tensors of this call, `inputs` = (name, tensor or
        None, dtype, shape) ..., into `req`, then the library's `call` on the current stream."""
        req.phases = int(phases)
        for name, t, dtype, shape in inputs:
            if t is not None:
                check_tensor(self.device, name, t, dtype, shape)
            setattr(req, name, _ptr(t))
        req.stream = self._stream().value
        _lib.check(call(self._h, C.byref(req)), self._h)

    def tree_request(self, tree: Dict[str, torch.Tensor], c_uct: float = 1.0) -> "_lib.PcbenvTreeRequest":
        """The request of `tree_advance` for the tensors in `tree` (see `pcbenv.search.new_tree` for a set of the right
        shapes): the keys are the members of pcbenv_tree_request -- `ln_dev`, the tree tensors `num_nodes` ... `best_actions`,
        `selected`, `path_len`, `paths` and optionally `errors_dev` -- on this device, contiguous, of the dtypes and shapes
        include/pcbenv.h gives; P, N, C and T are read off `children` [P, N, C] and `paths` [T, P, 3].  The request holds
        addresses only: the caller keeps the tensors alive."""
        i32, f64 = torch.int32, torch.float64
        ch, paths = tree["children"], tree["paths"]
        if ch.dim() != 3 or paths.dim() != 3 or paths.shape[1:] != (ch.shape[0], 3):
            raise ValueError(f"children must be [P, N, C] and paths [T, P, 3], got {tuple(ch.shape)} and {tuple(paths.shape)}")
        (P, N, Cc), T = ch.shape, paths.shape[0]
        want = {"ln_dev": (f64, (N + 1,)), "num_nodes": (i32, (P,)), "parent": (i32, (P, N)), "depth": (i32, (P, N)), "visits": (i32, (P, N)),
                "num_children": (i32, (P, N)), "node_action": (i32, (P, N, 3)), "children": (i32, (P, N, Cc)), "value_sum": (f64, (P, N)),
                "value_max": (f64, (P, N)), "terminal": (torch.uint8, (P, N)), "reward_lo": (f64, (P,)), "reward_hi": (f64, (P,)),
                "best_reward": (f64, (P,)), "best_length": (i32, (P,)), "best_actions": (i32, (T, P, 3)), **_exchange_want(T, P)}
        return self._tree_request(_lib.PcbenvTreeRequest, tree, want, num_roots=P, capacity=N, max_children=Cc, max_steps=T, c_uct=float(c_uct))

    def tree_advance(self, req: "_lib.PcbenvTreeRequest", phases: int, reward: Optional[torch.Tensor] = None,
                     length: Optional[torch.Tensor] = None, actions: Optional[torch.Tensor] = None) -> None:
        """One step of P search trees on the device (`pcbenv_tree_advance`, one kernel launch on the current stream, nothing
        else): `phases` is a set of `_lib.TREE_INIT`, `TREE_ABSORB`, `TREE_SELECT`, run in that order.  SELECT descends every
        tree by UCT and writes `selected`, `path_len` and `paths` -- the `paths=` / `path_len=` of the next `playout` call;
        ABSORB takes that playout's `reward` [P] float64, `length` [P] int32 and `actions` [T, P, 3] int32, expands and
        backs up.  `req`: `tree_request(tree, c_uct)`, reusable for every call on the same tensors."""
        P, T = req.num_roots, req.max_steps
        if P == 0:  # torch gives empty tensors a null pointer
            return
        self._advance(self._L.pcbenv_tree_advance, req, phases, (("reward", reward, torch.float64, (P,)), ("length", length, torch.int32, (P,)),
                                                                 ("actions", actions, torch.int32, (T, P, 3))))

    def _puct_absorb(self, call, req, R, phases, value, leaf_terminal, cand_count, cand_actions, cand_prior) -> None:
        """`puct_advance` and `puct_advance_leaves` past their empty batch: the ABSORB inputs, R rows of them."""
        K = int(cand_prior.shape[1]) if isinstance(cand_prior, torch.Tensor) and cand_prior.dim() == 2 else "K"
        req.num_candidates = K if isinstance(K, int) else 0
        self._advance(call, req, phases, (("value", value, torch.float64, (R,)), ("leaf_terminal", leaf_terminal, torch.uint8, (R,)),
                                          ("cand_count", cand_count, torch.int32, (R,)), ("cand_actions", cand_actions, torch.int32, (R, K, 3)),
                                          ("cand_prior", cand_prior, torch.float32, (R, K))))

    def puct_request(self, tree: Dict[str, torch.Tensor], c_puct: float = 1.0, max_children: int = 16) -> "_search_lib.PcbenvPuctRequest":
        """The request of `puct_advance` for the tensors in `tree` (see `pcbenv.search.new_puct_tree` for a set of the right
        shapes): the keys are the members of pcbenv_puct_request (include/pcbenv_search.h) -- the tree tensors `num_nodes`
        ... `reward_hi`, `selected`, `path_len`, `paths` and optionally `errors_dev` -- on this device, contiguous, of the
        dtypes and shapes the header gives; P, N and T are read off `parent` [P, N] and `paths` [T, P, 3], C = max_children
        is an argument (the tree has no tensor with that extent).  The request holds addresses only: the caller keeps the
        tensors alive."""
        par, paths = tree["parent"], tree["paths"]
        if par.dim() != 2 or paths.dim() != 3 or paths.shape[1:] != (par.shape[0], 3):
            raise ValueError(f"parent must be [P, N] and paths [T, P, 3], got {tuple(par.shape)} and {tuple(paths.shape)}")
        (P, N), T = par.shape, paths.shape[0]
        return self._tree_request(_search_lib.PcbenvPuctRequest, tree, _puct_tree_want(P, N, _exchange_want(T, P)), num_roots=P, capacity=N,
                                  max_children=int(max_children), max_steps=T, c_puct=float(c_puct))

    def puct_advance(self, req: "_search_lib.PcbenvPuctRequest", phases: int, value: Optional[torch.Tensor] = None,
                     leaf_terminal: Optional[torch.Tensor] = None, cand_count: Optional[torch.Tensor] = None,
                     cand_actions: Optional[torch.Tensor] = None, cand_prior: Optional[torch.Tensor] = None) -> None:
        """One step of P PUCT search trees on the device (`pcbenv_puct_advance`, one kernel launch on the current stream,
        nothing else): `phases` is a set of `_lib.TREE_INIT`, `TREE_ABSORB`, `TREE_SELECT`, run in that order.  SELECT descends
        every tree by q + c_puct * prior * sqrt(n) / (1 + n_c) and writes `selected`, `path_len` and `paths` -- the `paths=` /
        `path_len=` of the next `gather_` or `playout` call; ABSORB takes the evaluation of the selected nodes -- `value` [P]
        float64, `leaf_terminal` [P] uint8, `cand_count` [P] int32, `cand_actions` [P, K, 3] int32, `cand_prior` [P, K]
        float32; K is read off `cand_prior` -- expands and backs up.  `req`: `puct_request(tree, c_puct, max_children)`,
        reusable for every call on the same tensors."""
        P = req.num_roots
        if P == 0:  # torch gives empty tensors a null pointer
            return
        self._puct_absorb(self._L.pcbenv_puct_advance, req, P, phases, value, leaf_terminal, cand_count, cand_actions, cand_prior)

    def puct_leaves_request(self, tree: Dict[str, torch.Tensor], c_puct: float = 1.0, max_children: int = 16,
                            leaves: int = 1) -> "_leaves_lib.PcbenvPuctLeavesRequest":
        """The request of `puct_advance_leaves` for the tensors in `tree` (see `pcbenv.search.new_puct_tree(leaves=L)` for a
        set of the right shapes): the keys are the members of pcbenv_puct_leaves_request (include/pcbenv_leaves.h) -- the
        tree tensors `num_nodes` ... `reward_hi` and `pending`, `selected`, `path_len`, `paths` and optionally `errors_dev`
        -- on this device, contiguous, of the dtypes and shapes the header gives; P, N and T are read off `parent` [P, N]
        and `paths` [T, P * L, 3], C = max_children and L = leaves are arguments.  The request holds addresses only: the
        caller keeps the tensors alive."""
        par, paths, L = tree["parent"], tree["paths"], int(leaves)
        if L < 1 or L > _leaves_lib.MAX_PUCT_LEAVES:
            raise ValueError(f"leaves must be in [1, {_leaves_lib.MAX_PUCT_LEAVES}], got {L}")
        if par.dim() != 2 or paths.dim() != 3 or paths.shape[1:] != (par.shape[0] * L, 3):
            raise ValueError(f"parent must be [P, N] and paths [T, P * {L}, 3], got {tuple(par.shape)} and {tuple(paths.shape)}")
        (P, N), T = par.shape, paths.shape[0]
        want = _puct_tree_want(P, N, _exchange_want(T, P * L), slots=("pending",))
        return self._tree_request(_leaves_lib.PcbenvPuctLeavesRequest, tree, want, num_roots=P, capacity=N, max_children=int(max_children),
                                  max_steps=T, c_puct=float(c_puct), num_leaves=L)

    def puct_advance_leaves(self, req: "_leaves_lib.PcbenvPuctLeavesRequest", phases: int, value: Optional[torch.Tensor] = None,
                            leaf_terminal: Optional[torch.Tensor] = None, cand_count: Optional[torch.Tensor] = None,
                            cand_actions: Optional[torch.Tensor] = None, cand_prior: Optional[torch.Tensor] = None) -> None:
        """One step of P PUCT search trees with L = req.num_leaves leaves per root on the device
        (`pcbenv_puct_advance_leaves`, one kernel launch on the current stream, nothing else): `phases` is a set of
        `_lib.TREE_INIT`, `TREE_ABSORB`, `TREE_SELECT`, run in that order.  SELECT descends every tree L times, each descent
        leaving a pending visit on its path, and writes `selected`, `path_len` [P * L] and `paths` [T, P * L, 3], row
        p * L + l the leaf l of root p (-1 in `selected` and `path_len`: no leaf) -- the `paths=` / `path_len=` of the next
        `gather_` or `playout(k=L)` call; ABSORB takes the evaluation of those rows -- `value` [P * L] float64,
        `leaf_terminal` [P * L] uint8, `cand_count` [P * L] int32, `cand_actions` [P * L, K, 3] int32, `cand_prior`
        [P * L, K] float32; K is read off `cand_prior` -- expands and backs up, leaf after leaf.  `req`:
        `puct_leaves_request(tree, c_puct, max_children, leaves)`, reusable for every call on the same tensors."""
        P = req.num_roots
        if P == 0:  # torch gives empty tensors a null pointer
            return
        self._puct_absorb(self._L.pcbenv_puct_advance_leaves, req, P * req.num_leaves, phases, value, leaf_terminal, cand_count, cand_actions,
                          cand_prior)

    def frontier_request(self, tensors: Dict[str, torch.Tensor], width: int, num_candidates: int,
                         prior_weight: float = 0.0) -> "_frontier_lib.PcbenvFrontierRequest":
        """The request of `frontier_advance` for the tensors in `tensors` (see `pcbenv.search.new_frontier_tensors` for a set
        of the right shapes): the two sets of rows `paths_0`, `path_len_0`, `cum_logp_0` and `paths_1`, `path_len_1`,
        `cum_logp_1`, the members `parent_row`, `live`, `best_value`, `best_len`, `best_path` of pcbenv_frontier_request
        (include/pcbenv_frontier.h) and optionally `errors_dev` -- on this device, contiguous, of the dtypes and shapes the
        header gives; P and T are read off `best_path` [T, P, 3], W = width and K = num_candidates are arguments.  The
        request holds addresses only: the caller keeps the tensors alive."""
        W, K, best = int(width), int(num_candidates), tensors["best_path"]
        if W < 1 or W > _frontier_lib.MAX_FRONTIER_WIDTH or K < 1 or K > _frontier_lib.MAX_FRONTIER_CANDIDATES or W * K > _frontier_lib.MAX_FRONTIER_ROWS:
            raise ValueError(f"width and num_candidates must be in [1, 64] and their product at most {_frontier_lib.MAX_FRONTIER_ROWS}, got {W} and {K}")
        if best.dim() != 3 or best.shape[2] != 3:
            raise ValueError(f"best_path must be [T, P, 3], got {tuple(best.shape)}")
        T, P = int(best.shape[0]), int(best.shape[1])
        i32, f64, R = torch.int32, torch.float64, P * W * K
        want = {"parent_row": (i32, (R,)), "live": (i32, (P,)), "best_value": (f64, (P,)), "best_len": (i32, (P,)), "best_path": (i32, (T, P, 3))}
        req = self._tree_request(_frontier_lib.PcbenvFrontierRequest, tensors, want, num_roots=P, width=W, num_candidates=K, max_steps=T,
                                 prior_weight=float(prior_weight))
        sets = []
        for s in (0, 1):
            for name, (dtype, shape) in (("paths", (i32, (T, R, 3))), ("path_len", (i32, (R,))), ("cum_logp", (f64, (R,)))):
                check_tensor(self.device, f"{name}_{s}", tensors[f"{name}_{s}"], dtype, shape)
            sets.append({name: _ptr(tensors[f"{name}_{s}"]) for name in _frontier_lib.FRONTIER_SET})
        req.sets = sets  # the addresses of set 0 and set 1: `frontier_advance` names one `in` and the other `out`
        return req

    def frontier_advance(self, req: "_frontier_lib.PcbenvFrontierRequest", phases: int, evaluation=None, swap: bool = False) -> None:
        """One depth of P beam searches over placements on the device (`pcbenv_frontier_advance`, one kernel launch on the
        current stream, nothing else).  `phases` is `_frontier_lib.FRONTIER_INIT` or `FRONTIER_ADVANCE`.  swap=False reads
        set 0 of the request's tensors as `in` and writes set 1 as `out`; swap=True the other way round.  INIT writes the
        root row into the out set; ADVANCE takes `evaluation`, the `pcbenv.search.Evaluation` of the in rows -- `value`
        [P * W * K] float64, `terminal` uint8 or bool, `cand_count` int32, `cand_actions` [P * W * K, K, 3] int32,
        `cand_prior` [P * W * K, K] float32 -- records the best finished row per root in `best_value`, `best_len` and
        `best_path`, keeps the W best expandable rows and writes their children, at most W * K per root, into the out
        set: the `paths=` / `path_len=` of the next `gather_` or `playout(k=W * K)` call.  `req`: `frontier_request(...)`,
        reusable for every call on the same tensors."""
        P, K = req.num_roots, req.num_candidates
        if P == 0:  # torch gives empty tensors a null pointer
            return
        R = P * req.width * K
        for name in _frontier_lib.FRONTIER_SET:
            setattr(req, name + "_in", req.sets[1 if swap else 0][name])
            setattr(req, name + "_out", req.sets[0 if swap else 1][name])
        ev = evaluation
        over = None if ev is None else ev.terminal.view(torch.uint8) if ev.terminal.dtype == torch.bool else ev.terminal
        self._advance(self._L.pcbenv_frontier_advance, req, phases,
                      (("value", None if ev is None else ev.value, torch.float64, (R,)), ("leaf_terminal", over, torch.uint8, (R,)),
                       ("cand_count", None if ev is None else ev.cand_count, torch.int32, (R,)),
                       ("cand_actions", None if ev is None else ev.cand_actions, torch.int32, (R, K, 3)),
                       ("cand_prior", None if ev is None else ev.cand_prior, torch.float32, (R, K))))

    def frontier_sample_request(self, tensors: Dict[str, torch.Tensor], width: int, num_candidates: int, seed: int,
                                first_root: int = 0) -> "_frontier_sample_lib.PcbenvFrontierSampleRequest":
        """The request of `frontier_sample` for the tensors in `tensors` (see `pcbenv.search.new_frontier_sample_tensors` for
        a set of the right shapes): the tensors `frontier_request` takes, `gumbel_0` and `gumbel_1` float64 [P * W * K], the
        third member of the two sets of rows, and the sample set `set_len` [P * W], `set_gumbel`, `set_logp`, `set_value`
        float64 [P * W] and `set_path` [T, P * W, 3] of pcbenv_frontier_sample_request (include/pcbenv_frontier_sample.h)
        -- on this device, contiguous.  P and T are read off `best_path` [T, P, 3]; `seed` and `first_root`, the global
        index of root 0, name the draws.  The request holds addresses only: the caller keeps the tensors alive."""
        W, K, best = int(width), int(num_candidates), tensors["best_path"]
        if W < 1 or W > _frontier_lib.MAX_FRONTIER_WIDTH or K < 1 or K > _frontier_lib.MAX_FRONTIER_CANDIDATES or W * K > _frontier_lib.MAX_FRONTIER_ROWS:
            raise ValueError(f"width and num_candidates must be in [1, 64] and their product at most {_frontier_lib.MAX_FRONTIER_ROWS}, got {W} and {K}")
        if best.dim() != 3 or best.shape[2] != 3:
            raise ValueError(f"best_path must be [T, P, 3], got {tuple(best.shape)}")
        T, P = int(best.shape[0]), int(best.shape[1])
        i32, f64, R, S = torch.int32, torch.float64, P * W * K, P * W
        want = {"parent_row": (i32, (R,)), "live": (i32, (P,)), "best_value": (f64, (P,)), "best_len": (i32, (P,)), "best_path": (i32, (T, P, 3)),
                "set_len": (i32, (S,)), "set_gumbel": (f64, (S,)), "set_logp": (f64, (S,)), "set_value": (f64, (S,)), "set_path": (i32, (T, S, 3))}
        req = self._tree_request(_frontier_sample_lib.PcbenvFrontierSampleRequest, tensors, want, num_roots=P, width=W, num_candidates=K, max_steps=T,
                                 seed=int(seed) & (2 ** 64 - 1), first_root=int(first_root))
        sets = []
        for s in (0, 1):
            for name, (dtype, shape) in (("paths", (i32, (T, R, 3))), ("path_len", (i32, (R,))), ("cum_logp", (f64, (R,))), ("gumbel", (f64, (R,)))):
                check_tensor(self.device, f"{name}_{s}", tensors[f"{name}_{s}"], dtype, shape)
            sets.append({name: _ptr(tensors[f"{name}_{s}"]) for name in _frontier_sample_lib.SAMPLE_SET})
        req.sets = sets  # the addresses of set 0 and set 1: `frontier_sample` names one `in` and the other `out`
        return req

    def frontier_sample(self, req: "_frontier_sample_lib.PcbenvFrontierSampleRequest", phases: int, step_index: int, evaluation=None,
                        swap: bool = False) -> None:
        """One depth of P stochastic beam searches over placements on the device (`pcbenv_frontier_sample`, one kernel launch
        on the current stream, nothing else).  As `frontier_advance`, with the rows ordered by their perturbed
        log-probability `gumbel` in place of their value: ADVANCE keeps the W contenders with the largest one among the set
        entries, the finished rows -- which enter the sample set `set_*` -- and the expandable rows, whose children are
        written with a Gumbel of their own, drawn for (seed, first_root + p, `step_index`).  `req`:
        `frontier_sample_request(...)`, reusable for every call on the same tensors."""
        P, K = req.num_roots, req.num_candidates
        if P == 0:  # torch gives empty tensors a null pointer
            return
        R = P * req.width * K
        for name in _frontier_sample_lib.SAMPLE_SET:
            setattr(req, name + "_in", req.sets[1 if swap else 0][name])
            setattr(req, name + "_out", req.sets[0 if swap else 1][name])
        req.step_index = int(step_index) & (2 ** 64 - 1)
        ev = evaluation
        over = None if ev is None else ev.terminal.view(torch.uint8) if ev.terminal.dtype == torch.bool else ev.terminal
        self._advance(self._L.pcbenv_frontier_sample, req, phases,
                      (("value", None if ev is None else ev.value, torch.float64, (R,)), ("leaf_terminal", over, torch.uint8, (R,)),
                       ("cand_count", None if ev is None else ev.cand_count, torch.int32, (R,)),
                       ("cand_actions", None if ev is None else ev.cand_actions, torch.int32, (R, K, 3)),
                       ("cand_prior", None if ev is None else ev.cand_prior, torch.float32, (R, K))))

    def puct_move_request(self, tree: Dict[str, torch.Tensor], max_children: int = 16) -> "_move_lib.PcbenvPuctMoveRequest":
        """The request of `puct_move` for the tensors in `tree`: the tree tensors of `puct_request` (`num_nodes` ...
        `reward_hi`) and the members of pcbenv_puct_move_request (include/pcbenv_move.h) `move_slot` [P], `move_action`
        [P, 3], `child_visits` [P, C], `child_actions` [P, C, 3], `root_value` float64 [P], `remap` [P, N] and optionally
        `errors_dev` -- see `pcbenv.search.new_move_tensors` for a set of the right shapes -- on this device, contiguous, of
        the dtypes and shapes the header gives; P and N are read off `parent` [P, N], C = max_children is an argument.  The
        request holds addresses only: the caller keeps the tensors alive."""
        i32, f64 = torch.int32, torch.float64
        par = tree["parent"]
        if par.dim() != 2:
            raise ValueError(f"parent must be [P, N], got {tuple(par.shape)}")
        (P, N), Cn = par.shape, int(max_children)
        own = {"move_slot": (i32, (P,)), "move_action": (i32, (P, 3)), "child_visits": (i32, (P, Cn)), "child_actions": (i32, (P, Cn, 3)),
               "root_value": (f64, (P,)), "remap": (i32, (P, N))}
        return self._tree_request(_move_lib.PcbenvPuctMoveRequest, tree, _puct_tree_want(P, N, own), num_roots=P, capacity=N, max_children=Cn)

    def puct_move(self, req: "_move_lib.PcbenvPuctMoveRequest", phases: int, mode: int = _move_lib.MOVE_GREEDY, seed: Optional[int] = None,
                  step_index: int = 0, reset: Optional[torch.Tensor] = None) -> None:
        """The move of P PUCT trees on the device (`pcbenv_puct_move`, one kernel launch on the current stream, nothing
        else): `phases` is a set of `_move_lib.MOVE_CHOOSE` and `MOVE_REROOT`, run in that order.  CHOOSE writes the root's
        `child_visits`, `child_actions` and `root_value` and picks `move_slot` / `move_action`: the most-visited child
        (`MOVE_GREEDY`) or a child drawn in proportion to the visit counts (`MOVE_PROPORTIONAL`) with the library's draw
        hash of (seed, first_env_index + p, step_index); seed defaults to the environment's run_seed.  REROOT makes the
        subtree of `move_slot` the tree, in place, and writes `remap`; a root with `reset` [P] uint8 non-zero (or without
        children) gets an empty tree instead.  `req`: `puct_move_request(tree, max_children)`, reusable for every call on
        the same tensors."""
        P = req.num_roots
        if P == 0:  # torch gives empty tensors a null pointer
            return
        req.mode, req.seed = int(mode), (self.run_seed if seed is None else int(seed)) & (2 ** 64 - 1)
        req.step_index, req.first_root = int(step_index) & (2 ** 64 - 1), self.first_env_index
        self._advance(self._L.pcbenv_puct_move, req, phases, (("reset", reset, torch.uint8, (P,)),))

    def puct_noise_request(self, tree: Dict[str, torch.Tensor], max_children: int = 16) -> "_noise_lib.PcbenvPuctNoiseRequest":
        """The request of `puct_root_noise` for the tensors in `tree`: the members of pcbenv_puct_noise_request
        (include/pcbenv_noise.h) `num_children`, `first_child` [P, N] int32, `prior` [P, N] float64, `noised` [P] int32 and
        optionally `errors_dev` -- `pcbenv.search.new_puct_tree` has a set of the right shapes -- on this device,
        contiguous, of the dtypes and shapes the header gives; P and N are read off `prior` [P, N], C = max_children is an
        argument.  The request holds addresses only: the caller keeps the tensors alive."""
        i32 = torch.int32
        pri = tree["prior"]
        if pri.dim() != 2:
            raise ValueError(f"prior must be [P, N], got {tuple(pri.shape)}")
        P, N = pri.shape
        want = {"num_children": (i32, (P, N)), "first_child": (i32, (P, N)), "prior": (torch.float64, (P, N)), "noised": (i32, (P,))}
        return self._tree_request(_noise_lib.PcbenvPuctNoiseRequest, tree, want, num_roots=P, capacity=N, max_children=int(max_children))

    def puct_root_noise(self, req: "_noise_lib.PcbenvPuctNoiseRequest", alpha: float, eps: float, seed: Optional[int] = None,
                        step_index: int = 0) -> None:
        """Dirichlet noise on the root priors of P PUCT trees on the device (`pcbenv_puct_root_noise`, one kernel launch on
        the current stream, nothing else): every root with `noised` 0 and children gets prior = float32((1 - eps) * prior +
        eps * eta) on its children, eta a draw from Dir(alpha) keyed by the library's draw hash of (seed, first_env_index +
        p, step_index), and `noised` 1; seed defaults to the environment's run_seed.  alpha in [0.01, 100], eps in [0, 1].
        `req`: `puct_noise_request(tree, max_children)`, reusable for every call on the same tensors."""
        if req.num_roots == 0:  # torch gives empty tensors a null pointer
            return
        req.alpha, req.eps = float(alpha), float(eps)
        req.seed = (self.run_seed if seed is None else int(seed)) & (2 ** 64 - 1)
        req.step_index, req.first_root = int(step_index) & (2 ** 64 - 1), self.first_env_index
        req.stream = self._stream().value
        _lib.check(self._L.pcbenv_puct_root_noise(self._h, C.byref(req)), self._h)

    def gumbel_request(self, tree: Dict[str, torch.Tensor], c_puct: float = 1.0, max_children: int = 16, c_visit: float = 50.0,
                       c_scale: float = 1.0) -> "_gumbel_lib.PcbenvGumbelRequest":
        """The request of `gumbel_advance` for the tensors in `tree`: the tensors of `puct_request` (`num_nodes` ...
        `reward_hi`, `selected`, `path_len`, `paths`) and the members of pcbenv_gumbel_request (include/pcbenv_gumbel.h)
        `sim_index` [P], `sim_visits` [P, C], `considered` [Mc + 1, n], `move_slot` [P], `move_action` [P, 3], `child_weights`
        [P, C], `child_policy` float32 [P, C], `child_actions` [P, C, 3], `root_value` float64 [P] and optionally `errors_dev`
        -- `pcbenv.search.new_puct_tree` and `new_gumbel_tensors` have a set of the right shapes -- on this device,
        contiguous, of the dtypes and shapes the header gives; P, N and T are read off `parent` [P, N] and `paths` [T, P, 3],
        Mc = max_considered and n = num_simulations off `considered`, C = max_children is an argument.  The request holds
        addresses only: the caller keeps the tensors alive."""
        i32, f64 = torch.int32, torch.float64
        par, paths, table = tree["parent"], tree["paths"], tree["considered"]
        if par.dim() != 2 or paths.dim() != 3 or paths.shape[1:] != (par.shape[0], 3):
            raise ValueError(f"parent must be [P, N] and paths [T, P, 3], got {tuple(par.shape)} and {tuple(paths.shape)}")
        if table.dim() != 2 or table.shape[0] < 2 or table.shape[0] > _gumbel_lib.MAX_CONSIDERED + 1 or table.shape[1] < 1:
            raise ValueError(f"considered must be [Mc + 1, n] with Mc in [1, {_gumbel_lib.MAX_CONSIDERED}] and n >= 1, got {tuple(table.shape)}")
        (P, N), T, Cn, (rows, n) = par.shape, paths.shape[0], int(max_children), table.shape
        own = {**_exchange_want(T, P), "sim_index": (i32, (P,)), "sim_visits": (i32, (P, Cn)), "considered": (i32, (rows, n)), "move_slot": (i32, (P,)),
               "move_action": (i32, (P, 3)), "child_weights": (i32, (P, Cn)), "child_policy": (torch.float32, (P, Cn)),
               "child_actions": (i32, (P, Cn, 3)), "root_value": (f64, (P,))}
        return self._tree_request(_gumbel_lib.PcbenvGumbelRequest, tree, _puct_tree_want(P, N, own), num_roots=P, capacity=N, max_children=Cn,
                                  max_steps=T, num_simulations=n, max_considered=rows - 1, c_puct=float(c_puct), c_visit=float(c_visit),
                                  c_scale=float(c_scale))

    def gumbel_advance(self, req: "_gumbel_lib.PcbenvGumbelRequest", phases: int, value: Optional[torch.Tensor] = None,
                       leaf_terminal: Optional[torch.Tensor] = None, cand_count: Optional[torch.Tensor] = None,
                       cand_actions: Optional[torch.Tensor] = None, cand_prior: Optional[torch.Tensor] = None, seed: Optional[int] = None,
                       step_index: int = 0) -> None:
        """One step of P search trees whose root level is a Gumbel search with Sequential Halving on the device
        (`pcbenv_gumbel_advance`, one kernel launch on the current stream, nothing else): `phases` is a set of
        `_gumbel_lib.GUMBEL_BEGIN`, `GUMBEL_ABSORB`, `GUMBEL_SELECT`, `GUMBEL_CHOOSE`, run in that order.  BEGIN zeroes the
        budget of a move (`sim_index`, `sim_visits`); ABSORB is `puct_advance`'s, with the same inputs; SELECT descends
        every tree -- level 0 by the schedule in `considered` on g + logit + sigma(q) while `sim_index` < n, every other
        level by PUCT -- and writes `selected`, `path_len` and `paths`; CHOOSE writes the move (`move_slot`, `move_action`),
        the policy target softmax(logit + sigma(completed q)) (`child_policy`, and `child_weights` in units of 2^-24, which
        `evaluate_visits` takes as it takes visit counts), `child_actions` and `root_value`.  The Gumbel draws have the key
        (seed, first_env_index + p, step_index), the same for every launch of a move; seed defaults to the environment's
        run_seed.  `req`: `gumbel_request(tree, ...)`, reusable for every call on the same tensors."""
        P = req.num_roots
        if P == 0:  # torch gives empty tensors a null pointer
            return
        req.seed = (self.run_seed if seed is None else int(seed)) & (2 ** 64 - 1)
        req.step_index, req.first_root = int(step_index) & (2 ** 64 - 1), self.first_env_index
        self._puct_absorb(self._L.pcbenv_gumbel_advance, req, P, phases, value, leaf_terminal, cand_count, cand_actions, cand_prior)

    def gumbel_tree_advance(self, req: "_gumbel_lib.PcbenvGumbelRequest", phases: int, value: Optional[torch.Tensor] = None,
                            leaf_terminal: Optional[torch.Tensor] = None, cand_count: Optional[torch.Tensor] = None,
                            cand_actions: Optional[torch.Tensor] = None, cand_prior: Optional[torch.Tensor] = None, seed: Optional[int] = None,
                            step_index: int = 0) -> None:
        """`gumbel_advance` under the full Gumbel rule (`pcbenv_gumbel_tree_advance`, include/pcbenv_gumbel_tree.h, one
        kernel launch on the current stream, nothing else): the same request -- `gumbel_request(tree, ...)` -- phases,
        tensors and key.  SELECT goes, at level 0 once the budget is spent and at every level below the root, to the child
        with the largest pi'(c) - n_c / (1 + sum n), pi' = softmax(logit + sigma(completed q)) over the node's children; a
        child without a visit is completed with v_mix, the node's value under its prior, at the root too -- in SELECT's
        scores and in CHOOSE's policy target.  `req.c_puct` is not read."""
        P = req.num_roots
        if P == 0:  # torch gives empty tensors a null pointer
            return
        req.seed = (self.run_seed if seed is None else int(seed)) & (2 ** 64 - 1)
        req.step_index, req.first_root = int(step_index) & (2 ** 64 - 1), self.first_env_index
        self._puct_absorb(self._L.pcbenv_gumbel_tree_advance, req, P, phases, value, leaf_terminal, cand_count, cand_actions, cand_prior)

    def gumbel_leaves_request(self, tree: Dict[str, torch.Tensor], c_puct: float = 1.0, max_children: int = 16, c_visit: float = 50.0,
                              c_scale: float = 1.0, leaves: int = 1) -> "_gumbel_leaves_lib.PcbenvGumbelLeavesRequest":
        """The request of `gumbel_advance_leaves` for the tensors in `tree`: the tensors of `gumbel_request` and `pending`
        [P, N], the exchange tensors with the leaf extent of `puct_leaves_request` -- `selected`, `path_len` [P * L], `paths`
        [T, P * L, 3] -- the members of pcbenv_gumbel_leaves_request (include/pcbenv_gumbel_leaves.h);
        `pcbenv.search.new_puct_tree(leaves=L)` and `new_gumbel_tensors` have a set of the right shapes.  P, N and T are read
        off `parent` and `paths`, Mc and n off `considered`; C = max_children and L = leaves are arguments.  The request
        holds addresses only: the caller keeps the tensors alive."""
        i32, f64 = torch.int32, torch.float64
        par, paths, table, L = tree["parent"], tree["paths"], tree["considered"], int(leaves)
        if L < 1 or L > _leaves_lib.MAX_PUCT_LEAVES:
            raise ValueError(f"leaves must be in [1, {_leaves_lib.MAX_PUCT_LEAVES}], got {L}")
        if par.dim() != 2 or paths.dim() != 3 or paths.shape[1:] != (par.shape[0] * L, 3):
            raise ValueError(f"parent must be [P, N] and paths [T, P * {L}, 3], got {tuple(par.shape)} and {tuple(paths.shape)}")
        if table.dim() != 2 or table.shape[0] < 2 or table.shape[0] > _gumbel_lib.MAX_CONSIDERED + 1 or table.shape[1] < 1:
            raise ValueError(f"considered must be [Mc + 1, n] with Mc in [1, {_gumbel_lib.MAX_CONSIDERED}] and n >= 1, got {tuple(table.shape)}")
        (P, N), T, Cn, (rows, n) = par.shape, paths.shape[0], int(max_children), table.shape
        own = {**_exchange_want(T, P * L), "sim_index": (i32, (P,)), "sim_visits": (i32, (P, Cn)), "considered": (i32, (rows, n)), "move_slot": (i32, (P,)),
               "move_action": (i32, (P, 3)), "child_weights": (i32, (P, Cn)), "child_policy": (torch.float32, (P, Cn)),
               "child_actions": (i32, (P, Cn, 3)), "root_value": (f64, (P,))}
        return self._tree_request(_gumbel_leaves_lib.PcbenvGumbelLeavesRequest, tree, _puct_tree_want(P, N, own, slots=("pending",)), num_roots=P,
                                  capacity=N, max_children=Cn, max_steps=T, num_simulations=n, max_considered=rows - 1, c_puct=float(c_puct),
                                  c_visit=float(c_visit), c_scale=float(c_scale), num_leaves=L)

    def gumbel_advance_leaves(self, req: "_gumbel_leaves_lib.PcbenvGumbelLeavesRequest", phases: int, value: Optional[torch.Tensor] = None,
                              leaf_terminal: Optional[torch.Tensor] = None, cand_count: Optional[torch.Tensor] = None,
                              cand_actions: Optional[torch.Tensor] = None, cand_prior: Optional[torch.Tensor] = None, seed: Optional[int] = None,
                              step_index: int = 0) -> None:
        """`gumbel_advance` with L = req.num_leaves descents per root and launch (`pcbenv_gumbel_advance_leaves`, one kernel
        launch on the current stream, nothing else): the same phases and key.  SELECT takes up to L scheduled simulations
        of every root, one after the other along the schedule, each descent leaving a pending visit on its path, and
        writes `selected`, `path_len` [P * L] and `paths` [T, P * L, 3], row p * L + l the leaf l of root p, -1 in `selected`
        and `path_len` where there is no leaf: behind a repeat, which consumes no simulation, and behind the end of the
        budget.  ABSORB is `puct_advance_leaves`', with the same inputs of P * L rows.  BEGIN and CHOOSE are
        `gumbel_advance`'s.  `req`: `gumbel_leaves_request(tree, ...)`, reusable for every call on the same tensors."""
        P = req.num_roots
        if P == 0:  # torch gives empty tensors a null pointer
            return
        req.seed = (self.run_seed if seed is None else int(seed)) & (2 ** 64 - 1)
        req.step_index, req.first_root = int(step_index) & (2 ** 64 - 1), self.first_env_index
        self._puct_absorb(self._L.pcbenv_gumbel_advance_leaves, req, P * req.num_leaves, phases, value, leaf_terminal, cand_count, cand_actions,
                          cand_prior)

    def gumbel_tree_advance_leaves(self, req: "_gumbel_leaves_lib.PcbenvGumbelLeavesRequest", phases: int, value: Optional[torch.Tensor] = None,
                                   leaf_terminal: Optional[torch.Tensor] = None, cand_count: Optional[torch.Tensor] = None,
                                   cand_actions: Optional[torch.Tensor] = None, cand_prior: Optional[torch.Tensor] = None, seed: Optional[int] = None,
                                   step_index: int = 0) -> None:
        """`gumbel_advance_leaves` under the full Gumbel rule (`pcbenv_gumbel_tree_advance_leaves`,
        include/pcbenv_gumbel_tree_leaves.h, one kernel launch on the current stream, nothing else): the same request --
        `gumbel_leaves_request(tree, ...)` -- phases, tensors and key.  The scores of the root's children and CHOOSE's policy
        target are `gumbel_tree_advance`'s (v_mix completes a child without a visit); below the root, and at the root once
        the budget is spent, every descent goes to the child with the largest pi'(c) - (n_c + pending_c) / (1 + sum (n +
        pending)): a pending visit counts as a visit and enters nothing else, so pi' of a node is the same for all L leaves
        of a launch.  Repeats, the end of the budget and ABSORB are `gumbel_advance_leaves`'.  `req.c_puct` is not read."""
        P = req.num_roots
        if P == 0:  # torch gives empty tensors a null pointer
            return
        req.seed = (self.run_seed if seed is None else int(seed)) & (2 ** 64 - 1)
        req.step_index, req.first_root = int(step_index) & (2 ** 64 - 1), self.first_env_index
        self._puct_absorb(self._L.pcbenv_gumbel_tree_advance_leaves, req, P * req.num_leaves, phases, value, leaf_terminal, cand_count, cand_actions,
                          cand_prior)

    def top_priors(self, logits: torch.Tensor, K: int, mask_bits: Optional[torch.Tensor] = None,
                   out: Optional[Sequence[torch.Tensor]] = None, errors: Optional[torch.Tensor] = None):
        """The K largest legal logits of every row and their probabilities (`pcbenv_top_priors`, one kernel launch on the
        current stream): `(cand_count int32 [N], cand_actions int32 [N, K, 3], cand_prior float32 [N, K])`, the tensors
        `puct_advance` takes.  logits: float32 or bfloat16 `[N, A]`, A = O*H*W in the flat action order; illegal entries
        have no influence.  mask_bits: int64 `[N, 2, H, WW]` (what `mask_bits()` returns) for arbitrary rows; None: row e
        is environment e (N = num_envs) and the legal set is the current `action_mask`, read from the state on the
        device.  Candidates come by logit descending, ties by flat index; the prior is float32(exp(l - max) / sum) over the
        whole legal set, not renormalised over the K kept; entries behind cand_count are zero.  out: three tensors of
        those shapes to write into (every element is written).  errors: int32 [1] the error bits are ORed into (1: a
        legal logit was NaN or +inf, 2: every legal logit was -inf; those rows list their first legal actions with
        prior 1/n), or None.  See include/pcbenv_priors.h."""
        cfg, K = self.cfg, int(K)
        dtype = _logits_dtype(logits)
        N = logits.shape[0] if logits.dim() == 2 else "N"
        if mask_bits is None:
            N = self.num_envs
        check_tensor(self.device, "logits", logits, LOGITS_DTYPES, (N, cfg.num_orientations * cfg.height * cfg.width))
        if mask_bits is not None:
            check_tensor(self.device, "mask_bits", mask_bits, torch.int64, (N, 2, cfg.height, (cfg.width + 63) // 64))
        if errors is not None:
            check_tensor(self.device, "errors", errors, torch.int32, (1,))
        if out is None:
            out = (torch.empty(N, dtype=torch.int32, device=self.device), torch.empty((N, K, 3), dtype=torch.int32, device=self.device),
                   torch.empty((N, K), dtype=torch.float32, device=self.device))
        count, actions, prior = out
        for name, t, dt, shape in (("out[0] (cand_count)", count, torch.int32, (N,)), ("out[1] (cand_actions)", actions, torch.int32, (N, K, 3)),
                                   ("out[2] (cand_prior)", prior, torch.float32, (N, K))):
            check_tensor(self.device, name, t, dt, shape)
        if N == 0:  # torch gives empty tensors a null pointer
            return count, actions, prior
        R = _priors_lib.PcbenvTopPriorsRequest
        req = R(struct_size=C.sizeof(R), logits_dtype=dtype, num_candidates=K, reserved=0, num_rows=N, logits=logits.data_ptr(),
                mask_bits=_ptr(mask_bits), cand_count=count.data_ptr(), cand_actions=actions.data_ptr(), cand_prior=prior.data_ptr(),
                errors_dev=_ptr(errors), stream=self._stream().value)
        _lib.check(self._L.pcbenv_top_priors(self._h, C.byref(req)), self._h)
        return count, actions, prior

    def queue_cursors(self):
        """(min, max) over the environments of the number of resets performed so far (synchronises)."""
        lo, hi = C.c_uint32(), C.c_uint32()
        _lib.check(self._L.pcbenv_queue_cursors(self._h, C.byref(lo), C.byref(hi), self._stream()), self._h)
        return lo.value, hi.value

    # -- checkpoint / resume ------------------------------------------------------------------
    def state_dict(self) -> dict:
        """Library state + observation tensors (host copies).  The reference never serialises env state
        (SURVEY.md §5); this is what a resumable rollout needs.  With the on-device generator the blob also holds its
        streams, counters and queued records (a resumed run draws the same instances); a host-fed queue is reloaded
        separately."""
        n = self._L.pcbenv_state_bytes(self._h)
        buf = np.empty(n, np.uint8)
        _lib.check(self._L.pcbenv_get_state(self._h, buf.ctypes.data, self._stream()), self._h)
        stride = C.c_int64()
        self._L.pcbenv_mask_bits(self._h, C.byref(stride))
        nb = stride.value * self.num_envs  # the state blocks; the generator's section (if any) follows them
        d = {"state": buf[:nb], "generator": buf[nb:], "reward": self.reward.cpu(), "done": self.done.cpu(), "info": self.info_raw.cpu(),
             "last_done": self._last_done.cpu(), "slot": self.slot, "device_instances": self.device_instances}
        d.update({"obs/" + k: v.cpu() for k, v in self.obs.items()})
        return d

    def load_state_dict(self, d: dict):
        buf = np.ascontiguousarray(np.concatenate([np.asarray(d["state"], np.uint8).ravel(), np.asarray(d.get("generator", ()), np.uint8).ravel()]))
        if bool(d.get("device_instances", False)) != self.device_instances:
            raise ValueError("the checkpoint was taken with" + ("" if d.get("device_instances") else "out") + " the on-device generator: "
                             "call enable_device_instances() on this environment " + ("first" if d.get("device_instances") else "only after restoring"))
        if buf.size != self._L.pcbenv_state_bytes(self._h):
            raise ValueError("state size does not match this environment")
        if "slot" in d:
            self.select_slot(int(d["slot"]))
        _lib.check(self._L.pcbenv_set_state(self._h, buf.ctypes.data, self._stream()), self._h)
        self.reward.copy_(d["reward"]); self.done.copy_(d["done"]); self.info_raw.copy_(d["info"])
        for k, v in self.obs.items():
            v.copy_(d["obs/" + k])
        if self.mask_marginals:  # not part of a checkpoint: they summarise the mask that has just been restored
            am = self.obs["action_mask"].reshape(self.num_envs, -1, self.cfg.height, self.cfg.width)
            self.mask_marginals["rows"].copy_(am.amax(dim=3))
            self.mask_marginals["orientation"].copy_(am.amax(dim=(2, 3)))
        # `done` of the latest step: restored into the selected slot's tensor (where reset_done() will look)
        self._last_done = self.done
        if "last_done" in d:
            self._last_done.copy_(d["last_done"])

    def mask_bits(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Bit-packed legal-action mask, int64 [B, 2, H, ceil(W/64)] (a copy; bit y of word [b, o, x, y // 64]).
        out: a C-contiguous int64 tensor of that shape on `self.device` to write into instead (for example one step's
        row of a [T, B, 2, H, WW] trajectory tensor); it is returned."""
        H, WW = self.cfg.height, (self.cfg.width + 63) // 64
        if out is not None:  # before the library is asked for the block
            check_tensor(self.device, "out", out, torch.int64, (self.num_envs, 2, H, WW))
        stride = C.c_int64()
        ptr = self._L.pcbenv_mask_bits(self._h, C.byref(stride))
        raw = _as_tensor(ptr, stride.value * self.num_envs, self.device)  # library-owned block, wrapped without taking ownership
        rows = raw.view(self.num_envs, stride.value)[:, :2 * H * WW * 8]
        if out is None:
            return rows.contiguous().view(torch.int64).view(self.num_envs, 2, H, WW)
        out.view(torch.uint8).view(self.num_envs, 2 * H * WW * 8).copy_(rows)
        return out

    # reference-style attribute access
    @property
    def action_mask(self) -> torch.Tensor:
        return self.obs["action_mask"]

    @property
    def grid(self) -> torch.Tensor:
        return self.obs["grid"]
