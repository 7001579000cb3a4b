#!/usr/bin/env python3
"""Builds libpcbenv.so (HIP kernels + C ABI) for gfx950, in-tree.

hipcc cross-compiles without a GPU.  -ffp-contract=off: one IEEE operation per written operator (the reward path
must match the reference bit for bit).  The kernels of the four environment kinds are separate translation units
compiled in parallel -- csrc/pcb_kind.inc, csrc/pcb_playout.inc for pcbenv_playout and pcbenv_playout_paths, and
csrc/pcb_gather_paths.inc for pcbenv_gather_paths, each compiled once per row of UNITS below with that row's -D flags: the
kind (a template argument in the sources), the part and, for the second family of k_playout, PCB_PATHS -- then linked with
the host side -- the C ABI
(csrc/pcbenv_api.hip), the layout derivation (csrc/pcb_config.hip) and the on-device instance generator with its kernels
(csrc/pcb_gen.hip), which share csrc/pcb_host.h -- the two kernels every kind uses (csrc/pcb_sample.hip), the policy kernels
(csrc/pcb_policy*.hip), the tree steps with their entry points (csrc/pcb_tree.hip, and csrc/pcb_puct.hip
for include/pcbenv_search.h, csrc/pcb_puct_leaves.hip for include/pcbenv_leaves.h, csrc/pcb_puct_move.hip for include/pcbenv_move.h,
csrc/pcb_puct_noise.hip for include/pcbenv_noise.h, csrc/pcb_gumbel.hip for include/pcbenv_gumbel.h, csrc/pcb_gumbel_leaves.hip for include/pcbenv_gumbel_leaves.h, csrc/pcb_gumbel_tree.hip for include/pcbenv_gumbel_tree.h, csrc/pcb_gumbel_tree_leaves.hip for include/pcbenv_gumbel_tree_leaves.h, csrc/pcb_frontier.hip for include/pcbenv_frontier.h, csrc/pcb_frontier_sample.hip for include/pcbenv_frontier_sample.h;
what they share is csrc/pcb_group.h, the lane-group kernel skeleton and its launch, csrc/pcb_puct_group.h, the PUCT absorb
and descent of pcb_puct.hip and pcb_gumbel.hip, and csrc/pcb_tree_host.h, the argument checks of their entry points), the masked top-K of a policy's logits (csrc/pcb_top_priors.hip for include/pcbenv_priors.h)
and the host instance generator
(csrc/instance_gen.cpp).  csrc/pcb_layout.h is the layout contract both sides compile.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")


def unit(stem, source, kind, part=None, paths=False):
    """One row of UNITS: csrc/<source> compiled for one kind, part (pin kinds) and kernel family into <stem>_<kind>[_<part>].hip.o."""
    defs = [f"-DPCB_KIND=PCBENV_{kind.upper()}"] + ([f"-DPCB_PART={part}"] if part is not None else [])
    return (f"{stem}_{kind}" + (f"_{part}" if part is not None else "") + ".hip.o", source, ["-x", "hip"] + defs + (["-DPCB_PATHS=1"] if paths else []))


# The table of translation units: (object, source, flags of its own), slowest first.  What a part of a pin kind compiles
# is not said here: pcb_layout::step_build_part / playout_build_part / gather_paths_build_part (csrc/pcb_layout.h) decide
# it inside the source, and the host side calls exactly the parts some build maps to (csrc/pcb_launch.h launch_family).
PIN_KINDS, FLAT_KINDS = ("spatial", "pin"), ("rect", "square")
UNITS = ([unit("pcb_kind", "pcb_kind.inc", k) for k in FLAT_KINDS[::-1]]
         + [unit("pcb_kind", "pcb_kind.inc", k, p) for p in (2, 3, 0, 4, 1) for k in PIN_KINDS]
         + [unit("pcb_playout", "pcb_playout.inc", k, p) for p in (2, 1, 0) for k in PIN_KINDS]
         + [unit("pcb_playout", "pcb_playout.inc", k) for k in FLAT_KINDS]
         + [unit("pcb_playout_paths", "pcb_playout.inc", k, p, paths=True) for p in (2, 1, 0) for k in PIN_KINDS]
         + [unit("pcb_playout_paths", "pcb_playout.inc", k, paths=True) for k in FLAT_KINDS]
         + [unit("pcb_gather_paths", "pcb_gather_paths.inc", k, p) for p in (2, 1, 0) for k in PIN_KINDS]
         + [unit("pcb_gather_paths", "pcb_gather_paths.inc", k) for k in FLAT_KINDS]
         + [(u + ".o", u, []) for u in ("pcb_policy.hip", "pcb_policy_eval.hip", "pcb_policy_visits.hip", "pcb_policy_axis.hip", "pcb_tree.hip", "pcb_puct.hip", "pcb_puct_leaves.hip", "pcb_puct_move.hip", "pcb_puct_noise.hip", "pcb_gumbel.hip", "pcb_gumbel_leaves.hip", "pcb_gumbel_tree.hip", "pcb_gumbel_tree_leaves.hip", "pcb_frontier.hip", "pcb_frontier_sample.hip", "pcb_top_priors.hip", "pcb_gen.hip", "pcb_sample.hip",
                                        "pcbenv_api.hip", "pcb_config.hip", "instance_gen.cpp")])
DEPS = [os.path.join(REPO, "include", h) for h in ("pcbenv.h", "pcbenv_search.h", "pcbenv_priors.h", "pcbenv_move.h", "pcbenv_train.h", "pcbenv_leaves.h", "pcbenv_noise.h", "pcbenv_gumbel.h", "pcbenv_gumbel_leaves.h", "pcbenv_gumbel_tree.h", "pcbenv_gumbel_tree_leaves.h", "pcbenv_frontier.h", "pcbenv_frontier_sample.h")] + sorted(
    os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".inc", ".hip", ".cpp")))
OUT = os.path.join(HERE, "libpcbenv.so")
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-std=c++17", "-Wno-unused-value", "-pthread"]


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    raise RuntimeError("hipcc not found")


def build(force: bool = False, verbose: bool = False, out: str = OUT, extra_flags=(), jobs: int = 0) -> str:
    """`out` / `extra_flags`: diagnostic builds (tools/build_stamps.sh) next to the shipped library."""
    if not force and os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(s) for s in DEPS):
        return out
    objdir = os.path.join(HERE, "build", os.path.splitext(os.path.basename(out))[0])
    os.makedirs(objdir, exist_ok=True)
    cc, inc = hipcc(), ["-I", os.path.join(REPO, "include"), "-I", CSRC]

    def compile_one(unit):
        obj = os.path.join(objdir, unit[0])
        cmd = [cc] + FLAGS + list(extra_flags) + inc + unit[2] + ["-c", os.path.join(CSRC, unit[1]), "-o", obj]
        import time
        t0 = time.time()
        subprocess.check_call(cmd)
        if verbose:
            print(f"{time.time() - t0:6.1f} s  " + " ".join(cmd[len(FLAGS) + len(extra_flags) + len(inc) + 1:]), flush=True)
        return obj
    with ThreadPoolExecutor(max_workers=jobs or min(len(UNITS), os.cpu_count() or 1, 8)) as ex:
        objs = list(ex.map(compile_one, UNITS))
    cmd = [cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread", "-o", out] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return out


if __name__ == "__main__":
    flags = [a for a in sys.argv[1:] if a.startswith("-D")]
    outs = [a for a in sys.argv[1:] if a.endswith(".so")]
    print(build(force="--force" in sys.argv or bool(flags) or bool(outs), verbose=True, out=os.path.abspath(outs[0]) if outs else OUT, extra_flags=flags))
