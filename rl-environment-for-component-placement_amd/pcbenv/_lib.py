"""ctypes binding of libpcbenv.so (include/pcbenv.h).  No fallback: if the HIP
library is missing or does not load, importing the product fails loudly."""
from __future__ import annotations

import ctypes as C
import os

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("PCBENV_LIB", os.path.join(_PKG, "libpcbenv.so"))  # override: A/B builds only

PCBENV_OK, PCBENV_EINVAL, PCBENV_ELIMIT, PCBENV_EHIP, PCBENV_ESTATE = 0, -1, -2, -3, -4
ACTION_TUPLE, ACTION_FLAT = 0, 1
FLAG_INCREMENTAL_OBS = 1
FLAG_AUTO_RESET = 2
ABI_VERSION = 3
OPT_STREAM_THRESHOLD_BYTES, OPT_TERMINAL_TEAMS, OPT_GEN_GRID, OPT_GEN_LANES, OPT_FIXED_GEOMETRY = 1, 2, 3, 4, 5
LOGITS_F32, LOGITS_BF16 = 0, 1
DRAW_SAMPLE, DRAW_GREEDY = 0, 1
EVAL_ERR_NONFINITE, EVAL_ERR_ALL_NEG_INF, EVAL_ERR_ACTION = 1, 2, 4  # bits of pcbenv_evaluate_logits' *errors_dev
EVAL_ROW_OK, EVAL_ROW_ZERO, EVAL_ROW_NO_ONE_HOT = 0, 1, 2  # row status, stats[:, 3]
AXIS_ORIENTATION, AXIS_X, AXIS_Y = 0, 1, 2
AXIS_ERR_NONFINITE, AXIS_ERR_ALL_NEG_INF, AXIS_ERR_VALUE, AXIS_ERR_GIVEN = 1, 2, 4, 8  # bits of the axis entry points' *errors_dev
TREE_INIT, TREE_ABSORB, TREE_SELECT = 1, 2, 4  # phases of pcbenv_tree_advance
MAX_TREE_CHILDREN = 64
TREE_ERR_FULL, TREE_ERR_TREE = 1, 2  # bits of pcbenv_tree_advance's *errors_dev

EXPORTS = ("pcbenv_abi_version", "pcbenv_create", "pcbenv_destroy", "pcbenv_last_error",
           "pcbenv_instance_stride", "pcbenv_max_total_pins", "pcbenv_set_option", "pcbenv_bind_buffers", "pcbenv_bind_buffers_slots", "pcbenv_bind_compact_features", "pcbenv_select_slot",
           "pcbenv_load_instances", "pcbenv_reset", "pcbenv_step", "pcbenv_sample_actions", "pcbenv_step_sampled", "pcbenv_rollout_sampled",
           "pcbenv_mask_bits", "pcbenv_state_bytes", "pcbenv_get_state", "pcbenv_set_state", "pcbenv_queue_cursors",
           "pcbenv_instgen_device_enable", "pcbenv_instgen_device_status", "pcbenv_get_instances",
           "pcbenv_instgen_create", "pcbenv_instgen_destroy", "pcbenv_instgen_next", "pcbenv_instgen_next_batch",
           "pcbenv_gather", "pcbenv_sample_logits", "pcbenv_evaluate_logits", "pcbenv_evaluate_logits_backward",
           "pcbenv_sample_axis", "pcbenv_evaluate_axis", "pcbenv_evaluate_axis_backward", "pcbenv_playout", "pcbenv_playout_paths", "pcbenv_tree_advance",
           "pcbenv_gather_paths")


class PcbenvConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "kind", "height", "width", "min_component_w", "max_component_w", "min_component_h",
        "max_component_h", "max_num_components", "min_num_components", "net_distribution", "pin_spread",
        "min_num_nets", "max_num_nets", "max_num_pins_per_net", "min_num_pins_per_net", "reward_type",
        "reward_beam_width", "component_n")] + [
        ("weight_wirelength", C.c_double), ("weight_num_intersections", C.c_double),
        ("num_envs", C.c_int32), ("queue_depth", C.c_int32), ("flags", C.c_uint32), ("threads_per_env", C.c_int32)]


BUFFER_FIELDS = ("grid", "action_mask", "pin_grid", "component_grid", "all_components_feature",
                 "placement_mask", "component_mask", "all_pins_num_feature", "all_pins_cat_feature",
                 "reward", "done", "info", "mask_orientation", "mask_rows")


class PcbenvBuffers(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in BUFFER_FIELDS]


COMPACT_FIELDS = ("all_components_feature", "placement_mask", "component_mask", "all_pins_num_feature", "all_pins_cat_feature")


class PcbenvCompactFeatures(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in COMPACT_FIELDS]


class PcbenvPlayoutRequest(C.Structure):
    """pcbenv_playout_request (include/pcbenv.h), the arguments of pcbenv_playout_paths."""
    _fields_ = [("struct_size", C.c_uint32), ("action_format", C.c_int32), ("root_index_dev", C.c_void_p), ("num_playouts", C.c_int64),
                ("path_actions_dev", C.c_void_p), ("path_len_dev", C.c_void_p), ("path_steps", C.c_int32), ("max_steps", C.c_int32),
                ("reward_dev", C.c_void_p), ("done_dev", C.c_void_p), ("length_dev", C.c_void_p), ("info_dev", C.c_void_p),
                ("actions_out_dev", C.c_void_p), ("actions_steps", C.c_int32), ("leaf_mask_bits_dev", C.c_void_p), ("errors_dev", C.c_void_p),
                ("seed", C.c_uint64), ("first_env_index", C.c_uint64), ("step_index0", C.c_uint64), ("stream", C.c_void_p)]


class PcbenvGatherPathsRequest(C.Structure):
    """pcbenv_gather_paths_request (include/pcbenv.h), the arguments of pcbenv_gather_paths."""
    _fields_ = [("struct_size", C.c_uint32), ("action_format", C.c_int32), ("src", C.c_void_p), ("src_index_dev", C.c_void_p),
                ("path_actions_dev", C.c_void_p), ("path_len_dev", C.c_void_p), ("path_steps", C.c_int32), ("length_dev", C.c_void_p),
                ("errors_dev", C.c_void_p), ("stream", C.c_void_p)]


TREE_TENSORS = ("num_nodes", "parent", "depth", "visits", "num_children", "node_action", "children", "value_sum", "value_max", "terminal",
                "reward_lo", "reward_hi", "best_reward", "best_length", "best_actions")


class PcbenvTreeRequest(C.Structure):
    """pcbenv_tree_request (include/pcbenv.h), the arguments of pcbenv_tree_advance."""
    _fields_ = ([("struct_size", C.c_uint32), ("phases", C.c_int32), ("num_roots", C.c_int32), ("capacity", C.c_int32),
                 ("max_children", C.c_int32), ("max_steps", C.c_int32), ("c_uct", C.c_double), ("ln_dev", C.c_void_p)]
                + [(n, C.c_void_p) for n in TREE_TENSORS + ("selected", "path_len", "paths", "reward", "length", "actions", "errors_dev", "stream")])


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with "
                          f"`python rl-environment-for-component-placement_amd/build.py` (there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    L.pcbenv_abi_version.restype = C.c_int
    L.pcbenv_create.argtypes = [C.POINTER(PcbenvConfig), C.c_int, C.POINTER(C.c_void_p)]
    L.pcbenv_destroy.argtypes = [C.c_void_p]
    L.pcbenv_destroy.restype = None
    L.pcbenv_last_error.argtypes = [C.c_void_p]
    L.pcbenv_last_error.restype = C.c_char_p
    L.pcbenv_instance_stride.argtypes = [C.POINTER(PcbenvConfig)]
    L.pcbenv_instance_stride.restype = C.c_int64
    L.pcbenv_max_total_pins.argtypes = [C.POINTER(PcbenvConfig)]
    L.pcbenv_max_total_pins.restype = C.c_int32
    L.pcbenv_set_option.argtypes = [C.c_void_p, C.c_int32, C.c_int64]
    L.pcbenv_bind_buffers.argtypes = [C.c_void_p, C.POINTER(PcbenvBuffers)]
    L.pcbenv_bind_buffers_slots.argtypes = [C.c_void_p, C.POINTER(PcbenvBuffers), C.c_int32]
    L.pcbenv_select_slot.argtypes = [C.c_void_p, C.c_int32]
    L.pcbenv_bind_compact_features.argtypes = [C.c_void_p, C.POINTER(PcbenvCompactFeatures)]
    L.pcbenv_load_instances.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.pcbenv_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.pcbenv_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.pcbenv_sample_actions.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    L.pcbenv_step_sampled.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    L.pcbenv_state_bytes.argtypes = [C.c_void_p]
    L.pcbenv_state_bytes.restype = C.c_int64
    L.pcbenv_get_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.pcbenv_set_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.pcbenv_instgen_create.argtypes = [C.POINTER(PcbenvConfig), C.c_uint64, C.POINTER(C.c_void_p)]
    L.pcbenv_instgen_destroy.argtypes = [C.c_void_p]
    L.pcbenv_instgen_destroy.restype = None
    L.pcbenv_instgen_next.argtypes = [C.c_void_p, C.c_void_p]
    L.pcbenv_instgen_next_batch.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_void_p, C.c_int32]
    L.pcbenv_instgen_device_enable.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.pcbenv_instgen_device_status.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]
    L.pcbenv_get_instances.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.pcbenv_rollout_sampled.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    L.pcbenv_queue_cursors.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_void_p]
    L.pcbenv_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pcbenv_sample_logits.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    L.pcbenv_evaluate_logits.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pcbenv_evaluate_logits_backward.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pcbenv_sample_axis.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    L.pcbenv_evaluate_axis.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pcbenv_evaluate_axis_backward.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pcbenv_playout.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    L.pcbenv_playout_paths.argtypes = [C.c_void_p, C.POINTER(PcbenvPlayoutRequest)]
    L.pcbenv_tree_advance.argtypes = [C.c_void_p, C.POINTER(PcbenvTreeRequest)]
    L.pcbenv_gather_paths.argtypes = [C.c_void_p, C.POINTER(PcbenvGatherPathsRequest)]
    L.pcbenv_mask_bits.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.pcbenv_mask_bits.restype = C.c_void_p
    if L.pcbenv_abi_version() != ABI_VERSION:
        raise ImportError(f"libpcbenv.so ABI {L.pcbenv_abi_version()} != expected {ABI_VERSION}")
    _lib = L
    return L


def bind_exports(L, requests):
    """Prototypes `int name(handle, const request *)` on the loaded library for `requests`, {export name: request type}:
    what the bindings of the further headers (`_search_lib`, `_priors_lib`, `_move_lib`, `_train_lib`, `_leaves_lib`)
    share.  ImportError if the library lacks one (there is no fallback).  Returns L."""
    missing = [n for n in requests if not hasattr(L, n)]
    if missing:
        raise ImportError(f"libpcbenv.so lacks {missing}: rebuild it with `python rl-environment-for-component-placement_amd/build.py`")
    for name, request in requests.items():
        f = getattr(L, name)
        f.argtypes = [C.c_void_p, C.POINTER(request)]
        f.restype = C.c_int
    return L


def make_config(cfg, num_envs: int, queue_depth: int = 1, flags: int = 0) -> PcbenvConfig:
    c = PcbenvConfig()
    for name, _ in PcbenvConfig._fields_:
        if name == "reward_type":
            c.reward_type = cfg.reward_type_code
        elif name in ("num_envs", "queue_depth", "flags", "threads_per_env"):
            continue
        else:
            setattr(c, name, getattr(cfg, name))
    c.num_envs, c.queue_depth, c.flags = int(num_envs), int(queue_depth), int(flags)
    return c


class PcbenvError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libpcbenv error {code}: {msg}")
        self.code = code


def check(rc: int, handle=None):
    if rc == PCBENV_OK:
        return
    msg = load().pcbenv_last_error(handle).decode("utf-8", "replace")
    if rc in (PCBENV_EINVAL, PCBENV_ELIMIT):
        raise ValueError(msg)  # the reference raises ValueError for bad constructor parameters
    raise PcbenvError(rc, msg)
