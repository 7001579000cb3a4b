"""pcbenv_gather throughput: a full random permutation of the batch within one handle, mid-episode, timed with HIP events
after warm-up.  python tools/gather_bench.py [--reps N] [--cases c3:4096,c4:4096,c5:8192]

Algorithmic bytes per environment: 2 x stateStride (the source block read, the destination block written) plus one row of
every bound tensor written whole (observations, reward, done, info): c3 ~48.5 KB.  One JSON line per case: us per gather
(events around `reps` back-to-back gathers, which include the 25-byte-per-environment snapshot copies of reward / done /
info that a gather within one handle takes first) and that byte count over the time as a share of 8 TB/s."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rl-environment-for-component-placement_amd"))
import torch  # noqa: E402

from pcbenv import named_config  # noqa: E402
from pcbenv.batched_env import BatchedPlacementEnv  # noqa: E402


def bytes_per_env(env) -> int:
    stride = C.c_int64()
    env._L.pcbenv_mask_bits(env._h, C.byref(stride))
    rows = sum(v[0].numel() * v.element_size() // env.num_envs for v in env.traj.values())
    rows += sum(v[0].numel() * v.element_size() // env.num_envs for v in env.traj_marginals.values())
    info = 16 if env.info else 0
    return 2 * stride.value + rows + 8 + 1 + info


def run(name: str, B: int, reps: int, warmup: int):
    cfg = named_config(name)
    env = BatchedPlacementEnv(cfg, B, queue_depth=4, run_seed=1, auto_reset=True)
    env.enable_device_instances()
    env.reset()
    acts = torch.empty((B, 3), dtype=torch.int32, device=env.device)
    for t in range(cfg.max_num_components // 2):  # mid-episode: about half of the components placed
        env.rollout_step(t, out=acts)
    g = torch.Generator(device="cpu").manual_seed(0)
    perms = [torch.randperm(B, generator=g).to(device=env.device, dtype=torch.int32) for _ in range(4)]
    for i in range(warmup):
        env.gather_(perms[i % 4])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        env.gather_(perms[i % 4])
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    nb = bytes_per_env(env)
    out = {"config": name, "num_envs": B, "us_per_gather": round(us, 2), "bytes_per_env": nb,
           "tb_per_s": round(nb * B / us / 1e6, 3), "share_of_8tbps": round(nb * B / us / 1e6 / 8.0, 3), "reps": reps}
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cases", default="c3:4096,c4:4096,c5:8192")
    a = ap.parse_args()
    for case in a.cases.split(","):
        name, B = case.split(":")
        print(json.dumps(run(name, int(B), a.reps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
