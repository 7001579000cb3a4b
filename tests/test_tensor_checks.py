"""`check_tensor`, the one test every caller tensor passes before its address goes to a launch, and its use by the wrappers
of BatchedPlacementEnv: a tensor of the wrong dtype, shape, layout or device -- another GPU's included -- is refused with a
ValueError that names the argument, before anything reaches the library.  No device is needed: the device rule is
`torch.device` equality, and a shell without a handle stands in for an environment on cuda:1."""
import pytest
import torch

import logits_cases as lc
from pcbenv.batched_env import BatchedPlacementEnv, check_tensor

CPU = torch.device("cpu")


def test_the_right_tensor_passes():
    check_tensor(CPU, "x", torch.zeros((3, 5)), torch.float32, (3, 5))
    check_tensor(CPU, "x", torch.zeros((3, 5), dtype=torch.bfloat16), (torch.float32, torch.bfloat16), (3, 5))
    check_tensor(CPU, "x", torch.zeros(0, dtype=torch.int32), torch.int32, (0,))
    check_tensor(CPU, "x", torch.zeros((4, 3, 5))[1], torch.float32, [3, 5])   # a contiguous row of a larger tensor


@pytest.mark.parametrize("what, t", [
    ("dtype", torch.zeros((3, 5), dtype=torch.float64)),
    ("dtype of a tuple", torch.zeros((3, 5), dtype=torch.float16)),
    ("shape", torch.zeros((3, 6))),
    ("rank", torch.zeros(15)),
    ("strided view", torch.zeros((3, 10))[:, ::2]),
    ("transposed", torch.zeros((5, 3)).t()),
    ("not a tensor", [[0.0] * 5] * 3),
])
def test_a_wrong_tensor_is_refused_by_name(what, t):
    with pytest.raises(ValueError, match="my_argument") as e:
        check_tensor(CPU, "my_argument", t, (torch.float32, torch.bfloat16), (3, 5))
    for part in ("must have shape [3, 5]", "torch.float32 or torch.bfloat16", "C-contiguous", "must be on cpu"):
        assert part in str(e.value)


def test_a_size_that_could_not_be_read_matches_nothing():
    with pytest.raises(ValueError, match=r"must have shape \[N, 5\]"):
        check_tensor(CPU, "logits", torch.zeros(5), torch.float32, ("N", 5))


@pytest.mark.parametrize("want, have, ok", [("cuda:0", "cuda:0", True), ("cuda:0", "cuda:1", False), ("cuda:0", "cpu", False),
                                            ("cpu", "cuda:0", False), ("cuda:1", "cuda:1", True), ("cuda", "cuda:0", False)])
def test_the_device_rule_is_equality_index_included(want, have, ok):
    class OnDevice(torch.Tensor):  # a host tensor that reports `have`: no GPU is needed to state the rule
        device = torch.device(have)
    t = torch.zeros((2, 3)).as_subclass(OnDevice)
    if ok:
        check_tensor(torch.device(want), "x", t, torch.float32, (2, 3))
    else:
        with pytest.raises(ValueError, match=f"x: .*must be on {want}; got .* on {have}"):
            check_tensor(torch.device(want), "x", t, torch.float32, (2, 3))
    assert (torch.device(want) == torch.device(have)) == ok


class _Shell(BatchedPlacementEnv):
    """The wrappers' argument checks without a handle, as tests/test_factorised_cpu.py: whatever reached the library
    would fail on the missing `_L`, not with a ValueError."""

    def __init__(self, cfg, num_envs, device):
        self.cfg, self.num_envs, self.device, self._h = cfg, num_envs, torch.device(device), None


def _args(cfg, B):
    O, H, W = cfg.num_orientations, cfg.height, cfg.width
    return dict(O=O, H=H, W=W, flat=torch.zeros((B, O * H * W)), row=torch.zeros((B, H)), actions=torch.zeros((B, 3), dtype=torch.int32),
                bits=torch.zeros((B, 2, H, (W + 63) // 64), dtype=torch.int64))


def test_host_tensors_never_reach_the_library_of_a_handle_on_another_device():
    cfg, B = lc.RAGGED["spatial_7x100"](), 4
    env, a = _Shell(cfg, B, "cuda:1"), _args(cfg, B)
    assert env._h is None and not hasattr(env, "_L")
    calls = {
        "sample_logits": lambda: env.sample_logits(a["flat"], 0),
        "evaluate_logits_forward": lambda: env.evaluate_logits_forward(a["flat"], a["bits"], a["actions"]),
        "evaluate_logits_backward": lambda: env.evaluate_logits_backward(a["flat"], a["bits"], a["actions"], torch.zeros((B, 4)), None, None),
        "sample_axis": lambda: env.sample_axis(1, a["row"], 0, a["actions"], (0,)),
        "evaluate_axis_forward": lambda: env.evaluate_axis_forward(1, (0,), a["row"], a["bits"], a["actions"]),
        "evaluate_axis_backward": lambda: env.evaluate_axis_backward(1, (0,), a["row"], a["bits"], a["actions"], None, None),
        "tree_request": lambda: env.tree_request({"children": torch.zeros((2, 5, 3), dtype=torch.int32), "paths": torch.zeros((4, 2, 3), dtype=torch.int32),
                                                  "ln_dev": torch.zeros(6, dtype=torch.float64)}),
        "mask_bits": lambda: env.mask_bits(out=a["bits"]),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="must be on cuda:1"):
            call()


def test_every_tensor_of_a_call_is_checked_not_only_the_first():
    """On a shell whose device the tensors are on, each argument in turn is the one on the wrong device."""
    cfg, B = lc.RAGGED["spatial_7x100"](), 4
    env, a = _Shell(cfg, B, "cpu"), _args(cfg, B)

    class Elsewhere(torch.Tensor):
        device = torch.device("cuda:1")
    far = lambda t: t.as_subclass(Elsewhere)
    f32 = lambda *shape: torch.zeros(shape)
    cases = [
        ("actions", lambda: env.evaluate_logits_forward(a["flat"], a["bits"], far(a["actions"]))),
        ("mask_bits", lambda: env.evaluate_logits_forward(a["flat"], far(a["bits"]), a["actions"])),
        ("stats", lambda: env.evaluate_logits_forward(a["flat"], a["bits"], a["actions"], stats=far(f32(B, 4)))),
        ("stats", lambda: env.evaluate_logits_backward(a["flat"], a["bits"], a["actions"], far(f32(B, 4)), None, None)),
        ("grad_log_prob", lambda: env.evaluate_logits_backward(a["flat"], a["bits"], a["actions"], f32(B, 4), far(f32(B)), None)),
        ("grad_entropy", lambda: env.evaluate_logits_backward(a["flat"], a["bits"], a["actions"], f32(B, 4), None, far(f32(B)))),
        ("out must match", lambda: env.evaluate_logits_backward(a["flat"], a["bits"], a["actions"], f32(B, 4), None, None, out=far(f32(B, a["flat"].shape[1])))),
        ("actions", lambda: env.sample_axis(1, a["row"], 0, far(a["actions"]), (0,))),
        ("mask_bits", lambda: env.evaluate_axis_forward(1, (0,), a["row"], far(a["bits"]), a["actions"])),
        ("grad_entropy", lambda: env.evaluate_axis_backward(1, (0,), a["row"], a["bits"], a["actions"], None, far(f32(B)))),
        ("out must match", lambda: env.evaluate_axis_backward(1, (0,), a["row"], a["bits"], a["actions"], None, None, out=far(f32(B, a["H"])))),
        ("out", lambda: env.sample_logits(a["flat"], 0, out=far(a["actions"]))),
    ]
    for name, call in cases:
        with pytest.raises(ValueError, match=f"{name}.*must be on cpu"):
            call()


def test_sample_logits_out_is_checked():
    cfg, B = lc.RAGGED["spatial_7x100"](), 4
    env, a = _Shell(cfg, B, "cpu"), _args(cfg, B)
    bad = [("int64", False, torch.zeros((B, 3), dtype=torch.int64)), ("[B, 2]", False, torch.zeros((B, 2), dtype=torch.int32)),
           ("strided", False, torch.zeros((B, 6), dtype=torch.int32)[:, ::2]), ("[B, 3] for flat", True, torch.zeros((B, 3), dtype=torch.int32)),
           ("[B] for tuple", False, torch.zeros(B, dtype=torch.int32)), ("strided flat", True, torch.zeros(2 * B, dtype=torch.int32)[::2])]
    for what, flat, out in bad:
        for logits in (a["flat"], a["flat"].view(B, a["O"], a["H"], a["W"])):
            with pytest.raises(ValueError, match="out: must have shape"):
                env.sample_logits(logits, 0, flat=flat, out=out)


def test_mask_bits_out_is_refused_without_a_handle():
    cfg, B = lc.RAGGED["spatial_7x100"](), 4
    env, a = _Shell(cfg, B, "cpu"), _args(cfg, B)
    for out in (a["bits"].int(), a["bits"][:, :1], torch.zeros((B, 2, a["H"], 4), dtype=torch.int64)[..., ::2]):
        with pytest.raises(ValueError, match="out: must have shape"):
            env.mask_bits(out=out)
