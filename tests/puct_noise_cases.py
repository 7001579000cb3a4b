"""The cases of pcbenv_puct_root_noise (include/pcbenv_noise.h) and its CPU model: hand-built roots of every kind at every
group width, the calls made on them, and tools/puct_noise_check.cpp -- csrc/pcb_puct_noise.h as a program of its own,
built with AddressSanitizer and UBSan -- to run them.  tests/test_puct_noise_model.py holds the model to the
specification (pcbenv/search.py:puct_root_noise), tests/test_puct_noise_gpu.py the kernel to the model.

A case is P roots of N = 2 C + 4 slots.  Root p is of kind KINDS[p % len(KINDS)]:
  none   no children: left alone, noised stays 0       one    k = 1: eta is exactly 1
  full   k = C                                         part   1 < k < C (k = 1 at C = 3 ... whatever fits below C)
  done   k = C and noised already 1: left alone
Child ranges start at varying slots, every prior of the [P, N] tensor -- children or not -- is one of puct_cases.PRIORS, so
a store to a slot that is no child of the root shows.  Every case is called twice with the same arguments: the second call
is a no-op."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import model_harness as mh
import puct_cases as pc
from pcbenv.search import noise_base, noise_gammas

REPO = pc.REPO
ERR_TREE = 2
KINDS = ("full", "none", "one", "part", "done")
SEED = 0x5EED0123456789AB
BLOCK = 256

# name: (C, P, alpha, eps, first_root, step_index)
CASES = {
    "G4_C3_P67": (3, 67, 0.3, 0.25, 0, 77),                 # two workgroups of 64 roots, the second partly filled
    "G4_C4_P5": (4, 5, 1.0, 1.0, 3, 77),
    "G8_C8_P67": (8, 67, 2.5, 0.25, 11, (1 << 32) - 1),
    "G16_C16_P5": (16, 5, 0.03, 0.25, 0, (1 << 32) + 5),    # a step index past 2^32
    "G16_C16_P67": (16, 67, 0.3, 1.0, 1000, (1 << 40) + 1),
    "G32_C20_P5": (20, 5, 1.0, 0.25, 2, 0),
    "G64_C33_P5": (33, 5, 0.3, 0.0, 0, 77),                 # eps = 0: float32 priors stay as they are
    "G64_C64_P1": (64, 1, 2.5, 1.0, 7, 77),
    "G64_C64_P5": (64, 5, 0.03, 1.0, 0, 78),
}
DAMAGE_CASE, DAMAGE_ROOT = "G8_C8_P67", 10  # a root of kind "full" with neighbours on either side
# name: (tensor, value as a function of (N, k, C))
DAMAGE = {
    "more_children_than_C": ("num_children", lambda N, k, C: C + 1),
    "first_child_0": ("first_child", lambda N, k, C: 0),
    "first_child_past_the_end": ("first_child", lambda N, k, C: N - k + 1),
    "first_child_negative": ("first_child", lambda N, k, C: -(2 ** 31)),
    "children_int_max": ("num_children", lambda N, k, C: 2 ** 31 - 1),
}


def group_lanes(C):
    g = 4
    while g < C:
        g <<= 1
    return g


def program():
    """tools/puct_noise_check.cpp as tests/model_harness.py:tool builds it; None without g++."""
    return mh.tool("puct_noise_check")


def call(alpha, eps, seed=SEED, step_index=77, first_root=0):
    return dict(alpha=float(alpha), eps=float(eps), seed=seed, step_index=step_index, first_root=first_root)


def run(tree, C, seq):
    """tree: dict of num_children, first_child, prior [P, N] and noised [P] (numpy).  -> [state after call i]: dicts of prior
    float64 [P, N], noised int64 [P] and `errors`, the error bits of that call.  Raises on anything on stderr."""
    P, N = tree["prior"].shape
    words = [np.array([0, P, N, C, len(seq)], np.int64), tree["num_children"].astype(np.int64).ravel(), tree["first_child"].astype(np.int64).ravel(),
             mh.words(tree["prior"], True), tree["noised"].astype(np.int64).ravel()]
    for c in seq:
        words += [np.array([mh.u64(c["seed"]), mh.u64(c["step_index"]), c["first_root"], mh.bits(c["alpha"]), mh.bits(c["eps"])], np.int64)]
    return mh.cut(mh.run_words(program(), words), len(seq), ("prior", "noised"), {"prior": (P, N), "noised": (P,)}, ("prior",))


FUNCTIONS = ("ieee_ln", "ieee_exp", "ieee_sqrt")


def model_function(name, x):
    """csrc/pcb_ieee_math.h's function `name` of every element of x (float64), from the model program."""
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    pairs = np.stack([np.full(len(x), FUNCTIONS.index(name), np.int64), x.view(np.int64)], axis=1).ravel()
    return mh.run_words(program(), [np.array([1, len(x)], np.int64), pairs]).view(np.float64)


def part_children(C, p):
    """k of a root of kind "part": 1 < k < C where there is such a k."""
    return max(1, min(C - 1, 2 + p % max(1, C - 2)))


@functools.lru_cache(maxsize=None)
def case(name):
    """-> SimpleNamespace(name, P, N, C, G, kinds, k, tree, seq): the tensors of CASES[name] and its two calls."""
    C, P, alpha, eps, first_root, step_index = CASES[name]
    N = 2 * C + 4
    kinds = [KINDS[p % len(KINDS)] for p in range(P)]
    nchild, fchild = np.zeros((P, N), np.int32), np.full((P, N), -1, np.int32)
    noised = np.zeros(P, np.int32)
    prior = np.array([pc.PRIORS[(3 * p + s) % len(pc.PRIORS)] for p in range(P) for s in range(N)], np.float64).reshape(P, N)
    ks = np.zeros(P, np.int64)
    for p, kind in enumerate(kinds):
        k = {"none": 0, "one": 1, "full": C, "part": part_children(C, p), "done": C}[kind]
        fc = 1 + (p * 5) % (N - k) if k else -1  # 1 <= fc <= N - k, the last slot of the tree included now and then
        if kind == "full" and p % 2 == 0:
            fc = N - k
        nchild[p, 0], fchild[p, 0], ks[p] = k, fc, k
        noised[p] = 1 if kind == "done" else 0
        # below the root: nodes with children of their own, which are nobody's business here
        if k:
            nchild[p, fc], fchild[p, fc] = min(C, 2), 1
    tree = dict(num_children=nchild, first_child=fchild, prior=prior, noised=noised)
    seq = [call(alpha, eps, SEED, step_index, first_root)] * 2
    return SimpleNamespace(name=name, P=P, N=N, C=C, G=group_lanes(C), kinds=kinds, k=ks, tree=tree, seq=seq, alpha=alpha, eps=eps,
                           first_root=first_root, step_index=step_index)


def torch_tree(tree):
    return {f: torch.from_numpy(np.ascontiguousarray(v)) for f, v in tree.items()}


def damaged(name):
    """-> (the case, its tree with root DAMAGE_ROOT damaged, that root's index)."""
    c = case(DAMAGE_CASE)
    p = DAMAGE_ROOT
    assert c.kinds[p] == "full" and 0 < p < c.P - 1
    tensor, value = DAMAGE[name]
    tree = {f: np.array(v) for f, v in c.tree.items()}
    tree[tensor][p, 0] = value(c.N, int(c.k[p]), c.C)
    return c, tree, p


@functools.lru_cache(maxsize=None)
def check_cases():
    """The table is what it is there for: every group width, the root counts, every kind, both arms of the Gamma draw, every
    eps -- and, on the specification, no draw of the table exhausts its 32 attempts (a condition: the table's seed is
    chosen accordingly).  -> the cases."""
    cases = [case(n) for n in CASES]
    assert {c.G for c in cases} == {4, 8, 16, 32, 64} and {c.C for c in cases} >= {3, 4, 8, 16, 33, 64} and {c.P for c in cases} == {1, 5, 67}
    assert any(c.P % (BLOCK // c.G) for c in cases) and any(c.G == 4 and c.P > BLOCK // 4 for c in cases)
    assert {c.alpha for c in cases} == {0.03, 0.3, 1.0, 2.5} and {c.eps for c in cases} == {0.0, 0.25, 1.0}
    assert any(c.alpha < 1.0 for c in cases) and any(c.alpha >= 1.0 for c in cases)  # both arms
    assert any(c.first_root for c in cases) and any(c.step_index >> 32 for c in cases) and any(c.step_index < 1 << 32 for c in cases)
    for c in cases:
        if c.P >= len(KINDS):
            assert set(c.kinds) == set(KINDS)
        assert (c.k <= c.C).all() and (c.tree["first_child"][c.k > 0, 0] >= 1).all() and (c.tree["first_child"][:, 0] + c.k <= c.N).all()
        assert any(c.tree["first_child"][p, 0] + c.k[p] == c.N for p in range(c.P) if c.k[p])  # a range that ends with the tree
        rows = torch.arange(c.P, dtype=torch.int64) + c.first_root
        _, exhausted = noise_gammas(noise_base(SEED, rows, c.step_index)[:, None], torch.arange(c.C, dtype=torch.int64)[None, :], c.alpha)
        drawn = torch.arange(c.C)[None, :] < torch.from_numpy(c.k)[:, None]
        assert not bool((exhausted & drawn).any()), c.name
    assert any(c.C > 3 and ((c.k > 1) & (c.k < c.C)).any() for c in cases)
    return cases
