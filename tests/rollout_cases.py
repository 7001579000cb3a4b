"""Cases and the CPU plan of the persistent rollout, pcbenv_rollout_sampled (plain module, no test; needs no GPU).

A case is a handle configuration at a shape where the rollout build of k_step takes another path than at the named
configurations -- two mask words, four wavefronts, more rows than lanes, routes, beam width 4, in place, the generator at
its bound, one launch per step -- and a script: an ordered list of calls, ("rollout", n), ("fused",) = one rollout_step,
("step",) = an explicit step with the drawn actions, ("reset_mask", p).  `Plan` computes the whole script on the CPU
before any device call: a HandleModel stepped with the actions playout_cases.draw gives for (seed, first_env_index + i,
step) -- the sampling contract of include/pcbenv.h, not the kernel -- so that the expected actions, rewards, dones and
infos of every transition exist beforehand and a test can assert the mix of terminals a case needs.  The on-device
generator's records are the host streams', so the same plan serves device_instances=True.

In the trajectory layout every transition goes to the slot behind the one the last transition wrote: a call that steps
first selects slot + 1, and step t of a launch writes slot (selected + t) % S."""
import zlib
from functools import lru_cache

import numpy as np

from pcbenv import EnvConfig
from pcbenv.config import KIND_PIN, KIND_SPATIAL, KIND_SQUARE

import playout_cases as pc
from handle_model import HandleModel, Setup
from logits_cases import RAGGED

_CROWDED = (12, 12, 5, 5, 2, 5, 2, 5, 8, 8, 3, 5, 7, 2)  # tests/test_gpu_parity.py::test_no_legal_cell_terminals_with_in_launch_reset


def _script(lengths, routed_kind, tail=()):
    """The rollouts of `lengths` in order.  Behind the first: (for the pin kinds an explicit step, which runs with the
    helper teams the rollout's last step has listed environments for, and) a fused step, so that the second starts at
    the step index the fused launch has presampled.  Behind the second: a masked reset.  The others back to back, then
    the rollouts of `tail`."""
    calls = []
    for i, n in enumerate(tuple(lengths) + tuple(tail)):
        calls.append(("rollout", n))
        if i == 0:
            calls += ([("step",)] if routed_kind else []) + [("fused",)]
        elif i == 1:
            calls.append(("reset_mask", 0.5))
    return tuple(calls)


class Case:
    def __init__(self, name, cfg, kw, B, S, Q, seed, lengths, tail=(), device_instances=False):
        self.name, self.cfg, self.kw, self.B, self.S, self.Q, self.seed = name, cfg, dict(kw), B, S, Q, seed
        self.lengths, self.tail, self.device_instances = tuple(lengths), tuple(tail), device_instances
        self.script = _script(lengths, cfg().kind in (KIND_PIN, KIND_SPATIAL), tail)

    def setup(self):
        """The handle of the case as handle_model.Driver builds it."""
        kw = dict(self.kw, num_slots=self.S) if self.S > 1 else dict(self.kw)
        return Setup(self.name, self.cfg, self.B, (self.seed,), len(self.script), auto_reset=True, queue_depth=self.Q,
                     device_instances=self.device_instances, replay=False, **kw)


# The seeds: the first of 3, 2, 6 at which the plan of the case holds every condition of `conditions` (`pick_seed`, no
# device).  `tail`: rollouts behind the lengths of the table, each no longer than S, where those lengths alone leave more
# than half of the transitions in slots a later step of the same launch overwrites, or no launch without such a step.
CASES = {c.name: c for c in (
    # WW = 2, NW = 4, routed; padding bits behind column 100
    Case("spatial_7x100_t256", RAGGED["spatial_7x100"], {"threads_per_env": 256}, 12, 4, 8, 3, (5, 1, 7, 3)),
    # the feature cache filled by an in-launch reset and copied by later steps of the launch; marginals in every slot
    Case("spatial_7x100_compact", RAGGED["spatial_7x100"], {"compact_features": True, "mask_marginals": True}, 12, 4, 8, 3, (5, 1, 7, 3)),
    # 100 rows on 64 lanes: the fold is staged in LDS
    Case("pin_100x9", RAGGED["pin_100x9"], {}, 12, 5, 8, 3, (6, 9, 4)),
    # the pin kind with NW = 4 and routes, beam width 4, W not a power of two
    Case("pin_40x48_k4_t256", RAGGED["pin_40x48"], {"threads_per_env": 256, "compact_features": True}, 12, 4, 8, 3, (6, 9, 5), tail=(3,)),
    # one valid bit in word 1; 40 components; the slots wrap seven times in one launch
    Case("rect_33x65", RAGGED["rect_33x65"], {}, 8, 4, 8, 3, (9, 30, 12), tail=(4,) * 7),
    # the square kind at WW = 2; an episode is 42 placements (Q is unused: the square kind has no instance queue)
    Case("square_3x128", RAGGED["square_3x128"], {}, 4, 3, 1, 3, (30, 1, 20), tail=(3,) * 12),
    # worst-case terminals ("no legal cell left") mid-launch on four wavefronts
    Case("crowded_spatial_t256", lambda: EnvConfig.spatial(*_CROWDED, "both", 2, 0.5), {"threads_per_env": 256}, 16, 3, 8, 3, (7, 7, 7), tail=(3,)),
    # the in-place rollout (row-incremental features inside the loop) with a routed `beam` reward
    Case("crowded_pin_inplace", lambda: EnvConfig.pin(*_CROWDED, "beam", 2, 0.5), {}, 16, 1, 8, 3, (2, 3, 1, 4, 2, 3, 1, 4)),
    # placements 64 or more wide over both words; the host queue wraps inside a launch
    Case("rect_128_huge_inplace", lambda: EnvConfig.rect(128, 128, 1, 128, 1, 128, 6, 1), {}, 6, 1, 2, 3, (3, 2, 4, 1, 3)),
    # every transition is terminal: a launch consumes exactly num_steps records per environment, the generator's bound
    Case("rect_4x4_generator", lambda: EnvConfig.rect(4, 4, 4, 4, 4, 4, 2, 2), {}, 8, 3, 4, 3, (4, 4, 4, 3), device_instances=True),
    # 128 rows, 64 components, up to 256 pins on 64 lanes; nothing overwritten (n <= S)
    Case("spatial_max_t64", pc._spatial_max, {"threads_per_env": 64}, 3, 8, 2, 3, (8,) * 9),
    # PCBENV_FLAG_INCREMENTAL_OBS: one launch per step, actions at actions_out + t * B * 3
    Case("small_pin_incremental", lambda: EnvConfig.pin(10, 10, 3, 4, 2, 4, 2, 4, 6, 1, 2, 4, 5, 2, "centroid", 2, 0.5),
         {"incremental_obs": True}, 8, 1, 8, 3, (3, 5, 2, 4)),
)}
TWO_TERMINALS_IN_A_LAUNCH = ("spatial_7x100_t256", "pin_100x9", "rect_33x65", "crowded_spatial_t256", "rect_4x4_generator")
CROWDED = ("crowded_spatial_t256", "crowded_pin_inplace")


def call_seed(name, index):
    """The seed of call `index` of the script of case `name` (a masked reset draws its mask from it)."""
    return zlib.crc32(f"{name}:{index}".encode()) & 0x3FFFFFFF


def reset_mask(B, p, seed):
    """The mask Driver.op_reset_mask draws."""
    return (np.random.RandomState(seed).rand(B) < p).astype(np.uint8)


def draws(cfg, model, seed, first_env_index, step):
    """The actions pcbenv_sample_actions draws for every row of a HandleModel, int32 [B, 3]."""
    return np.stack([pc.draw(cfg, model.ob.env(i), seed, first_env_index + i, step) for i in range(model.B)])


class Plan:
    """The script of a case (or `script`) computed on the CPU.  calls[j]: dict(op, arg, seed, t0 = the step index of the
    call's first transition, slot0 = the slot it writes, actions int32 [n, B, 3], steps = [(reward, done, info)] per
    transition, mask = the reset mask)."""

    def __init__(self, case, script=None, seed=None, first_env_index=0):
        if isinstance(case, str):
            case = CASES[case]
        self.case, self.cfg = case, case.cfg()
        self.seed = case.seed if seed is None else seed
        cfg, B, S = self.cfg, case.B, case.S
        m = self.model = HandleModel(cfg, B, S, case.Q, True, self.seed, case.device_instances)
        m.reset()
        self.calls, t = [], 0
        for j, call in enumerate(case.script if script is None else script):
            op, arg = call[0], (call[1] if len(call) > 1 else 0)
            rec = dict(op=op, arg=arg, seed=call_seed(case.name, j), t0=t, slot0=m.slot, actions=None, steps=[], mask=None)
            if op == "reset_mask":
                rec["mask"] = reset_mask(B, arg, rec["seed"])
                m.reset(rec["mask"])
            else:
                n = arg if op == "rollout" else 1
                if S > 1:
                    m.select(m.slot + 1)
                rec["slot0"] = m.slot
                acts = np.zeros((n, B, 3), np.int32)
                for k in range(n):
                    acts[k] = draws(cfg, m, self.seed, first_env_index, t + k)
                    rr, dd, ii = m.step(acts[k], slot=(m.slot + k) % S, set_last_done=op != "rollout")
                    rec["steps"].append((np.array(rr, np.float64), np.array(dd, np.uint8), np.array(ii, np.float64)))
                rec["actions"] = acts
                if n:
                    m.select(m.slot + n - 1)
                t += n
            self.calls.append(rec)

    def digest(self):
        """Everything the plan expects, as bytes."""
        out = []
        for c in self.calls:
            out.append(repr((c["op"], c["arg"], c["seed"], c["t0"], c["slot0"])).encode())
            if c["mask"] is not None:
                out.append(c["mask"].tobytes())
            if c["actions"] is not None:
                out.append(c["actions"].tobytes())
            for rr, dd, ii in c["steps"]:
                out += [rr.tobytes(), dd.tobytes(), np.where(np.isnan(ii), -1.0, ii).tobytes(), np.isnan(ii).tobytes()]
        return b"".join(out)

    def mix(self):
        """Counts over the plan.  A launch is a ("rollout", n) call; `mid_*`: terminal at step k < n - 1 of a launch, so
        that the same launch steps the new episode; `twice`: (launch, environment) pairs with two or more terminals;
        `presample_hits`: launches directly behind a fused call, whose presampled action is the one of their step 0;
        `launches`: (n, steps whose slot a later step of the same launch overwrites) per launch."""
        cfg, B, S = self.cfg, self.case.B, self.case.S
        has_info = cfg.kind in (KIND_PIN, KIND_SPATIAL)
        mx = dict(transitions=0, terminals=0, routed=0, worst=0, ends=0, mid_launch=0, mid_routed=0, mid_worst=0, twice=0,
                  presample_hits=0, launches=[], uncompared=0, every_transition_terminal=True)
        prev = None
        for c in self.calls:
            n = len(c["steps"])
            per_env = np.zeros(B, np.int64)
            for k, (rr, dd, ii) in enumerate(c["steps"]):
                d = dd.astype(bool)
                worst = d & (ii[:, 0] == cfg.max_wirelength) & (ii[:, 1] == cfg.max_num_intersections) if has_info else np.zeros(B, bool)
                routed = d & ~worst if has_info else np.zeros(B, bool)
                mid = c["op"] == "rollout" and k < n - 1
                mx["transitions"] += B
                mx["terminals"] += int(d.sum())
                mx["routed"] += int(routed.sum())
                mx["worst"] += int(worst.sum())
                mx["ends"] += 0 if has_info else int(d.sum())
                mx["every_transition_terminal"] &= bool(d.all())
                if mid:
                    mx["mid_launch"] += int(d.sum())
                    mx["mid_routed"] += int(routed.sum())
                    mx["mid_worst"] += int(worst.sum())
                per_env += d
            if c["op"] == "rollout":
                over = max(n - S, 0)
                mx["launches"].append((n, over))
                mx["uncompared"] += over * B
                mx["twice"] += int((per_env >= 2).sum())
                mx["presample_hits"] += int(prev is not None and prev["op"] == "fused" and prev["t0"] + 1 == c["t0"] and n > 0)
            prev = c
        return mx


def conditions(case, mx):
    """What tests/test_rollout_cases.py asserts of a case's mix -> {condition: holds}."""
    name, kind = case.name, case.cfg().kind
    need = {"a presample hit at t = 0": mx["presample_hits"] >= 1}
    if name != "small_pin_incremental":  # (it has no persistent launch)
        need["a mid-launch terminal"] = mx["mid_launch"] >= 1
    if name in TWO_TERMINALS_IN_A_LAUNCH:
        need["an environment with two terminals in one launch"] = mx["twice"] >= 1
    if name in CROWDED:
        need["5 worst-case terminals mid-launch"] = mx["mid_worst"] >= 5
        need["5 routed terminals mid-launch"] = mx["mid_routed"] >= 5
    elif kind in (KIND_PIN, KIND_SPATIAL):
        need["a routed terminal"] = mx["routed"] >= 1
    if name == "rect_4x4_generator":
        need["every environment terminal at every step"] = mx["every_transition_terminal"] and mx["terminals"] == mx["transitions"]
    if case.S > 1:
        need["at most half of the transitions uncompared"] = 2 * mx["uncompared"] <= mx["transitions"]
        need["a launch with n <= S"] = any(0 < n <= case.S for n, _ in mx["launches"])
    return need


def pick_seed(name, seeds=(3, 2, 6)):
    """The first seed at which the case holds every condition (None: none of them does) and the conditions missed per seed."""
    missed = {}
    for s in seeds:
        need = conditions(CASES[name], Plan(name, seed=s).mix())
        missed[s] = [k for k, v in need.items() if not v]
        if not missed[s]:
            return s, missed
    return None, missed


@lru_cache(maxsize=None)
def plan(name):
    """The plan of a case, computed once and shared: nothing may change it."""
    return Plan(name)
