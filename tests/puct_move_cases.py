"""Cases and the CPU model of pcbenv_puct_move (plain module, no test; needs no GPU).

A case is the final tree of a recorded search of tests/puct_cases.py -- `synthetic(...)`, or for the chain the evaluator
below -- and, per root, a move of one of eight kinds by p % 8 (KINDS).  `run` feeds a tree and a sequence of calls to
tools/puct_move_check.cpp -- csrc/pcb_puct_move.h compiled for the CPU with AddressSanitizer and UBSan, a program of its
own -- and returns the state after every call.  `ways` are the three call sequences every case is run in; `damaged` are the
trees a caller has written out-of-range values into.  The GPU tests compare the kernel with the model's states.

Shapes (SHAPES): N = 31 is less than a 64-slot chunk; N = 161 and N = 331 have a ragged last chunk at C = 16 and C = 33; C =
64 with one root has N = 641, more than ten chunks; the chain is a C = 1 tree, T = 70, 80 iterations: every parent is the
previous slot (the previous lane of the kernel) and the chain crosses a chunk boundary; P = 9, 35 and 130 are several
workgroups of four roots with the last partly filled.

Constructed shapes (CONSTRUCTED): searched trees of ten iterations end before a third span of 256 slots, so a seeded
generator (Grower) makes well-formed trees of up to five spans -- a C = 1 chain of 700 slots, a chain of 63 links inside
one chunk, a C = 64 tree whose moved-to child was expanded two spans above itself, trees grown in random order whose kept
and dropped slots alternate in every chunk, and trees that fill N = 256, 257 and 512 to the last slot.  `coverage` counts,
from a tree and its moves alone, where pass 1 of REROOT finds every verdict it has to ask for; `check_constructed` asserts
what each shape is there for.  `damaged_deep` damages the third span of two of them."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import model_harness as mh
import puct_cases as pc
import sampling_contract as sc
from model_harness import flat, words as _words  # noqa: F401  (the tests take them from here)
from pcbenv.search import Evaluation

REPO = pc.REPO
CHOOSE, REROOT = 1, 2
GREEDY, PROPORTIONAL = 0, 1
ERR_TREE = 2
FILL = -7  # what the model's output tensors hold before the first call
TREE_FIELDS = pc.TREE_FIELDS
MOVE_FIELDS = ("move_slot", "move_action", "child_visits", "child_actions", "root_value", "remap")
STATE_FIELDS = MOVE_FIELDS + TREE_FIELDS
FLOATS = pc.FLOATS + ("root_value",)
POKED = ("move_slot", "num_nodes", "parent", "num_children", "first_child")  # the tensors a call's pokes may name, by number
KINDS = ("most_visited", "zero_visits", "grandchild", "slot_0", "minus_1", "reset", "last_slot", "proportional")
SEED, STEP, FIRST_ROOT = 0x5EED0123456789AB, 77, 3


def shapes(P, N, C):
    s = {"move_slot": (P,), "move_action": (P, 3), "child_visits": (P, C), "child_actions": (P, C, 3), "root_value": (P,), "remap": (P, N),
         "num_nodes": (P,), "node_action": (P, N, 3), "reward_lo": (P,), "reward_hi": (P,)}
    s.update({n: (P, N) for n in ("parent", "depth", "visits", "num_children", "first_child", "prior", "value_sum", "value_max", "terminal")})
    return s


def program():
    """tools/puct_move_check.cpp as tests/model_harness.py:tool builds it; None without g++."""
    return mh.tool("puct_move_check")


def call(phases, mode=GREEDY, move_slot=None, reset=None, pokes=(), seed=SEED, step_index=STEP, first_root=FIRST_ROOT):
    return dict(phases=phases, mode=mode, move_slot=move_slot, reset=reset, pokes=tuple(pokes), seed=seed, step_index=step_index, first_root=first_root)


def run(tree, C, seq):
    """tree: dict of TREE_FIELDS (numpy).  -> [state after call i]: dicts of STATE_FIELDS (int64; FLOATS as float64) and
    `errors`, the error bits of that call.  Raises on anything on stderr."""
    P, N = tree["parent"].shape
    parts = [np.array([P, N, C, len(seq)], np.int64)] + [_words(tree[f], f in FLOATS) for f in TREE_FIELDS]
    for c in seq:
        parts.append(np.array([c["phases"], c["mode"], mh.u64(c["seed"]), c["step_index"], c["first_root"], int(c["move_slot"] is not None),
                               int(c["reset"] is not None), len(c["pokes"])] + [w for name, at, value in c["pokes"] for w in (POKED.index(name), at, value)], np.int64))
        parts += [_words(c[f]) for f in ("move_slot", "reset") if c[f] is not None]
    return mh.cut(mh.run_words(program(), parts), len(seq), STATE_FIELDS, shapes(P, N, C), FLOATS)


# ---- the trees -----------------------------------------------------------------------------------------------------
def chain_evaluator(P, T):
    """One candidate per node and no end before depth T: the tree of every root is a chain."""
    def evaluate(paths, path_len, step_index0):
        plen = path_len.numpy()
        value = np.array([(0.25, 0.5, 0.75)[pc._mix(5, p, plen[p]) % 3] for p in range(P)])
        actions = np.zeros((P, 1, 3), np.int32)
        actions[:, 0, 2] = plen % 7
        return Evaluation(torch.from_numpy(value), torch.from_numpy((plen == T).astype(np.uint8)), torch.ones(P, dtype=torch.int32),
                          torch.from_numpy(actions), torch.full((P, 1), 0.5, dtype=torch.float32))
    return evaluate


# name: P, T, C, K, iterations (synthetic), or "chain"
SHAPES = {
    "G4_C3_P130": (130, pc.WIDTH_T, 3, 3, 10),     # N = 31: less than a chunk; 33 workgroups, the last half filled
    "G16_C16_P35": (35, pc.WIDTH_T, 16, 16, 10),   # N = 161: ragged last chunk
    "G64_C33_P9": (9, pc.WIDTH_T, 33, 33, 10),     # N = 331
    "G64_C64_P1": (1, pc.WIDTH_T, 64, 64, 10),     # N = 641: more than ten chunks, one root
    "chain_C1_T70": (3, 70, 1, 1, 80),             # N = 81: every parent is the previous slot, across the chunk boundary at 64
}


@functools.lru_cache(maxsize=None)
def searched(name):
    """-> (the PuctSearch of the shape's recorded search, C)."""
    P, T, C, K, iterations = SHAPES[name]
    if name.startswith("chain"):
        ps, _ = pc.record(P, T, iterations, 1.25, C, chain_evaluator(P, T), step_index=100)
        return ps, C
    return pc.synthetic(P, T, C, K, iterations).ps, C


def tree_of(ps):
    return {f: getattr(ps, f).numpy().copy() for f in TREE_FIELDS}


def subtree(tree, p, m):
    """The slots of the subtree of m in root p, in slot order (a walk over the child ranges)."""
    todo, out = [m], []
    while todo:
        s = todo.pop()
        out.append(s)
        todo += [int(tree["first_child"][p, s]) + c for c in range(int(tree["num_children"][p, s]))]
    return sorted(out)


def proportional_pick(visits, seed, genv, step):
    """The contract's draw restated with tests/sampling_contract.py: the least c whose inclusive prefix sum exceeds (hi32 * total) >> 32."""
    total = int(sum(int(v) for v in visits))
    at = (sc.hi32(seed, genv, step) * total) >> 32
    prefix = 0
    for c, v in enumerate(visits):
        prefix += int(v)
        if prefix > at:
            return c
    raise AssertionError("no visits to draw from")


def greedy_pick(visits):
    return int(np.argmax(np.asarray(visits)))  # the first maximum


def assign(tree, p, C, kind=None):
    """-> (kind, move_slot, reset) of root p: the kind asked for (p % 8 of KINDS unless given) where the tree has such a node,
    most_visited (or -1 for a root without children) otherwise."""
    n, k, fc = int(tree["num_nodes"][p]), int(tree["num_children"][p, 0]), int(tree["first_child"][p, 0])
    kind = KINDS[p % 8] if kind is None else kind
    if k == 0:
        kind = kind if kind in ("slot_0", "minus_1", "reset") else "minus_1"
        return kind, 0 if kind != "minus_1" else -1, int(kind == "reset")
    visits = tree["visits"][p, fc:fc + k]
    best = fc + greedy_pick(visits)
    if kind == "zero_visits":
        zero = [s for s in range(1, n) if tree["visits"][p, s] == 0]
        if zero:
            return kind, zero[0], 0
    elif kind == "grandchild":
        if tree["num_children"][p, best] > 0:
            return kind, int(tree["first_child"][p, best]), 0
    elif kind == "slot_0":
        return kind, 0, 0
    elif kind == "minus_1":
        return kind, -1, 0
    elif kind == "reset":
        return kind, best, 1
    elif kind == "last_slot":
        return kind, n - 1, 0
    elif kind == "proportional" and visits.sum() > 0:
        return kind, fc + proportional_pick(visits, SEED, FIRST_ROOT + p, STEP), 0
    return "most_visited", best, 0


@functools.lru_cache(maxsize=None)
def case(name):
    """-> SimpleNamespace(name, P, N, C, tree, kinds, move_slot int32 [P], reset uint8 [P], kept [P]: nodes each root keeps, mode)."""
    if name in CONSTRUCTED:
        return constructed_case(name)
    ps, C = searched(name)
    tree = tree_of(ps)
    P, N = tree["parent"].shape
    assert N == 1 + SHAPES[name][4] * C and int(ps.errors) == 0
    kinds, move, reset = zip(*(assign(tree, p, C) for p in range(P)))
    kept = [0 if reset[p] or move[p] < 0 else len(subtree(tree, p, move[p])) for p in range(P)]
    mode = PROPORTIONAL if list(SHAPES).index(name) % 2 else GREEDY
    return SimpleNamespace(name=name, P=P, N=N, C=C, tree=tree, kinds=kinds, move_slot=np.array(move, np.int32), reset=np.array(reset, np.uint8),
                           kept=kept, mode=mode)


def check_cases():
    """What the set of cases is there for: every kind of move occurs, one root keeps more than 1 + C nodes and one exactly 1;
    the shapes are the ones the module's docstring names."""
    cases = [case(n) for n in SHAPES]
    assert {k for c in cases for k in c.kinds} == set(KINDS)
    assert any(k > 1 + c.C for c in cases for k in c.kept) and any(k == 1 for c in cases for k in c.kept)
    assert [c.N for c in cases] == [31, 161, 331, 641, 81] and [c.P for c in cases] == [130, 35, 9, 1, 3]
    chain = case("chain_C1_T70")
    n = int(chain.tree["num_nodes"][0])
    assert n > 64 and (chain.tree["parent"][0, 1:n] == np.arange(n - 1)).all()  # every parent is the previous slot, past slot 64
    assert any(k > 64 for k in chain.kept)  # and a kept chain crosses the chunk boundary
    assert {c.mode for c in cases} == {GREEDY, PROPORTIONAL}
    return cases


# ---- constructed trees: many spans, which a search of ten iterations never fills --------------------------------------
# REROOT needs a well-formed tree, not a searched one.  A Grower makes one root's: parent(s) < s, the children of a node in
# consecutive slots made at once, and -- filled in from the leaves up by a hash of (seed, root, slot) -- visits, values and
# priors from the small exact sets of tests/puct_cases.py, a node's visits 1 + its children's; unused slots hold INIT values.
LANES, SPAN = 64, 256  # csrc/pcb_puct_move.hip: the slots of one load of a wavefront, and the UNROLL = 4 of them it holds at a time
OUT, IN, ASK_PARENT = 0, 1, 2


def kept_at_sight(s, m, parent):
    """csrc/pcb_puct_move.h:kept_at_sight."""
    return IN if s == m else OUT if (s < m or parent < m) else IN if parent == m else ASK_PARENT


class Grower:
    def __init__(self, N, C):
        self.N, self.C = N, C
        self.parent, self.depth, self.k, self.fc, self.no = [-1], [0], [0], [-1], [0]

    @property
    def n(self):
        return len(self.parent)

    def expand(self, s, k):
        assert 0 <= s < self.n and self.k[s] == 0 and 1 <= k <= self.C and self.n + k <= self.N, (s, k, self.n)
        self.fc[s], self.k[s] = self.n, k
        for c in range(k):
            self.parent.append(s); self.depth.append(self.depth[s] + 1); self.k.append(0); self.fc.append(-1); self.no.append(c)
        return self

    def below(self, s, m):
        while s > m:
            s = self.parent[s]
        return s == m

    def grow(self, rng, n, under=0):
        """Random expansion order: a random leaf (below `under`) gets 1 .. C children, until n slots are in use."""
        while self.n < n:
            leaves = [s for s in range(self.n) if self.k[s] == 0 and self.below(s, under)]
            self.expand(leaves[rng.randint(len(leaves))], min(1 + rng.randint(self.C), n - self.n))
        return self

    def rows(self, seed, p):
        n, N, inf = self.n, self.N, float("inf")
        t = dict(parent=np.full(N, -1, np.int64), depth=np.zeros(N, np.int64), visits=np.zeros(N, np.int64), num_children=np.zeros(N, np.int64),
                 first_child=np.full(N, -1, np.int64), node_action=np.zeros((N, 3), np.int32), prior=np.zeros(N), value_sum=np.zeros(N),
                 value_max=np.full(N, -inf), terminal=np.zeros(N, np.bool_))
        t["parent"][:n], t["depth"][:n], t["num_children"][:n], t["first_child"][:n] = self.parent, self.depth, self.k, self.fc
        for s in reversed(range(n)):
            h = pc._mix(seed, p, s)
            v = (0.25, 0.5, 0.75)[(h >> 16) % 3]
            if self.k[s] == 0:
                visits = (h >> 8) % 4
                t["visits"][s], t["value_sum"][s], t["value_max"][s] = visits, visits * v, v if visits else -inf
                t["terminal"][s] = visits > 0 and (h >> 24) % 5 == 0
            else:
                ch = slice(self.fc[s], self.fc[s] + self.k[s])
                t["visits"][s], t["value_sum"][s] = 1 + t["visits"][ch].sum(), v + t["value_sum"][ch].sum()
                t["value_max"][s] = max(v, t["value_max"][ch].max())
            if s:
                t["prior"][s], t["node_action"][s] = pc.PRIORS[(h >> 32) % len(pc.PRIORS)], ((h >> 40) % 2, 0, self.no[s])
        return t


def _chain(N, n):
    g = Grower(N, 1)
    for s in range(n - 1):
        g.expand(s, 1)
    return g


def _chunk_chain(N, n, rng, under):
    """Slots 0 .. 63 a random binary tree; slots 64 .. 127 one chain below a leaf of the subtree of `under`, a child of the root:
    lane l of the chunk has lane l - 1 as its parent, 63 links; random again from there."""
    g = Grower(N, 2).expand(0, 2).grow(rng, LANES)
    g.expand(max(s for s in range(LANES) if g.k[s] == 0 and g.below(s, under)), 1)
    for s in range(LANES, 2 * LANES - 1):
        g.expand(s, 1)
    return g.grow(rng, n)


def _wide(N, m, steps):
    """C = 64.  The root's child m is expanded late, after seven of its siblings: its children are slots 513 .. 576, two spans
    above it; theirs follow, in the same span behind an earlier chunk (577 .., 897 ..) and in later spans (705 .. 768, 769 ..,
    961 .. 1024, 1025 ..), between ranges that are not kept.  steps: how much of that is made."""
    g = Grower(N, 64).expand(0, 64)
    others = [c for c in range(1, 9) if c != m][:7]
    script = [(s, 64) for s in others] + [(m, 64), (513, 64), (65, 64), (514, 64), (577, 64), (66, 64), (769, 64), (578, 64), (770, 64), (1025, 33)]
    for s, k in script[:steps]:
        g.expand(s, k)
    return g


def _random(N, C, n, rng):
    return Grower(N, C).expand(0, 2).grow(rng, n)


def _long_chain():
    N = 3 * SPAN + 1  # three full spans and a one-slot fourth
    return N, 1, [(_chain(N, 700), 1), (_chain(N, N), 256), (_chain(N, 690), 255), (_chain(N, 513), 257), (_chain(N, 700), 600),
                  (_chain(N, 300), "last_slot"), (_chain(N, 700), "reset"), (_chain(N, 641), "minus_1"), (_chain(N, 520), "slot_0"),
                  (_chain(N, 600), "grandchild"), (_chain(N, 700), "most_visited")]


def _full_chunk_chain():
    N, rng = 3 * LANES + 1, np.random.RandomState(64)
    return N, 2, [(_chunk_chain(N, 190, rng, 1), 1), (_chunk_chain(N, N, rng, 2), 1), (_chunk_chain(N, 150, rng, 1), "grandchild"),
                  (_chunk_chain(N, 2 * LANES, rng, 1), 1), (_chunk_chain(N, 181, rng, 2), "reset"), (_chunk_chain(N, 180, rng, 2), 2)]


def _wide_shape():
    N = 5 * SPAN + 1
    return N, 64, [(_wide(N, 5, 17), 5), (_wide(N, 5, 17), 5), (_wide(N, 5, 12), 5), (_wide(N, 9, 17), 9), (_wide(N, 5, 17), "grandchild"),
                   (_wide(N, 5, 16), "reset"), (_wide(N, 5, 15), 5)]


def _by_turns(N, C, n, rng):
    """Random expansion order, by turns below the root's first and second child: either subtree has slots everywhere."""
    g, turn = Grower(N, C).expand(0, 2), 0
    while g.n < n:
        g.grow(rng, min(n, g.n + 1 + rng.randint(C)), under=1 + turn % 2)
        turn += 1
    return g


def _interleaved():
    N, rng = 4 * SPAN + 77, np.random.RandomState(5)
    return N, 5, [(_by_turns(N, 5, 1000, rng), 1), (_by_turns(N, 5, N, rng), 2), (_by_turns(N, 5, 777, rng), 1),
                  (_by_turns(N, 5, 1000, rng), "proportional"), (_random(N, 5, 900, rng), "zero_visits"), (_by_turns(N, 5, 1040, rng), 2)]


def _edge(N, counts, seed):
    rng = np.random.RandomState(seed)
    kinds = ("half", "half", "proportional", "last_slot", "half", "grandchild", "half")
    return N, 5, [(_random(N, 5, n, rng), kinds[p]) for p, n in enumerate(counts)]


# name: -> N, C, [(the Grower of root p, its move: a slot, a kind of KINDS, or "half": the root's child that keeps nearest to half the tree)]
CONSTRUCTED = {
    "long_chain": _long_chain,
    "full_chunk_chain": _full_chunk_chain,
    "wide": _wide_shape,
    "interleaved": _interleaved,
    "edge_N256": lambda: _edge(256, (200, 256, 256, 129, 64, 255), 256),   # a full tree: the last span is exactly full
    "edge_N512": lambda: _edge(512, (300, 512, 512, 511, 257, 450), 512),
    "edge_N257": lambda: _edge(257, (256, 257, 100, 193, 257, 255, 130), 257),  # one slot in the second span
}
ALL_SHAPES = tuple(SHAPES) + tuple(CONSTRUCTED)
CONSTRUCTED_SEED = 23


@functools.lru_cache(maxsize=None)
def constructed_case(name):
    N, C, roots = CONSTRUCTED[name]()
    P = len(roots)
    rows = [g.rows(CONSTRUCTED_SEED + list(CONSTRUCTED).index(name), p) for p, (g, _) in enumerate(roots)]
    tree = {f: np.stack([r[f] for r in rows]) for f in rows[0]}
    tree.update(num_nodes=np.array([g.n for g, _ in roots], np.int64), reward_lo=np.full(P, 0.25), reward_hi=np.full(P, 0.75))
    tree = {f: tree[f] for f in TREE_FIELDS}
    kinds, move, reset = [], [], []
    for p, (g, spec) in enumerate(roots):
        if spec == "half":
            sizes = [len(subtree(tree, p, 1 + c)) for c in range(g.k[0])]
            spec = 1 + int(np.argmin([abs(2 * k - g.n) for k in sizes]))
        kind, m, r = ("given", spec, 0) if isinstance(spec, int) else assign(tree, p, C, spec)
        kinds.append(kind); move.append(m); reset.append(r)
    kept = [0 if reset[p] or move[p] < 0 else len(subtree(tree, p, move[p])) for p in range(P)]
    mode = PROPORTIONAL if list(CONSTRUCTED).index(name) % 2 else GREEDY
    return SimpleNamespace(name=name, P=P, N=N, C=C, tree=tree, kinds=tuple(kinds), move_slot=np.array(move, np.int32), reset=np.array(reset, np.uint8),
                           kept=kept, mode=mode)


def coverage(c, move_slot=None):
    """Where pass 1 of REROOT (csrc/pcb_puct_move.hip) finds the verdict of every used slot above the move that has to ask for
    its parent's, counted from the tree and the moves (c.move_slot: the `given_move` way) alone; and what else a shape is there for."""
    move_slot = c.move_slot if move_slot is None else move_slot
    out = SimpleNamespace(below_kept=[], below_dropped=0, earlier_kept=0, earlier_dropped=0, same_chunk=0, longest=0, crossings=set(), low_start=[],
                          full=[], mixed={}, num_nodes=[int(n) for n in c.tree["num_nodes"]])
    for p in range(c.P):
        n, m, par = int(c.tree["num_nodes"][p]), int(move_slot[p]), c.tree["parent"][p]
        if n == c.N:
            out.full.append(p)
        if c.reset[p] or m <= 0:  # an empty tree, or the identity: no pass 1
            continue
        keep = set(subtree(c.tree, p, m))
        if len(keep) < m and len(keep) // LANES < m // LANES:  # pass 3 starts at min(count, m) & ~63
            out.low_start.append((p, len(keep), m))
        links = {}
        for s in range(m + 1, n):
            up = int(par[s])
            if kept_at_sight(s, m, up) != ASK_PARENT:
                continue
            if up < s // SPAN * SPAN:
                if s in keep:
                    out.below_kept.append((p, s // SPAN))
                else:
                    out.below_dropped += 1
            elif up < s // LANES * LANES:
                out.earlier_kept += s in keep
                out.earlier_dropped += s not in keep
            else:
                out.same_chunk += 1
                links[s] = links.get(up, 0) + 1
                out.longest = max(out.longest, links[s])
        for B in (SPAN, 2 * SPAN):  # a kept link over the boundary, with kept links on either side of it
            if any(s >= B > par[s] > m and c.tree["num_children"][p, s] > 0 for s in keep):
                out.crossings.add((p, B))
        chunks = range(m // LANES + 1, n // LANES)  # the whole chunks above the move's
        if all(0 < sum(s in keep for s in range(k * LANES, (k + 1) * LANES)) < LANES for k in chunks):
            out.mixed[p] = len({k * LANES // SPAN for k in chunks})  # in how many spans
    return out


def check_constructed():
    """What the constructed shapes are there for, asserted on the CPU.  -> {name: coverage}."""
    cov = {name: coverage(case(name)) for name in CONSTRUCTED}
    for name, v in cov.items():
        c = case(name)
        assert c.P >= 6 and c.P % 4 != 0 and len(set(v.num_nodes)) >= 4, name  # a partly filled last workgroup; wavefronts of different lengths
        assert all(c.kinds[p] in ("given", "most_visited", "grandchild", "proportional") and v.num_nodes[p] < c.N for p in (0, c.P - 1)), name
    below = [(name, p, span) for name, v in cov.items() for p, span in v.below_kept]
    assert len(below) >= 64 and len({span for _, _, span in below}) >= 3 and len({(name, p) for name, p, _ in below}) >= 3
    assert all(len([1 for _, span in cov["wide"].below_kept if span == k]) >= 64 for k in (3, 4))  # the verdict comes out of remap in spans 3 and 4
    assert cov["wide"].earlier_kept >= 64 and all(v.earlier_kept > 0 for name, v in cov.items() if name != "long_chain")
    assert cov["full_chunk_chain"].longest == LANES - 1 and cov["long_chain"].longest == LANES - 1
    assert any({(p, SPAN), (p, 2 * SPAN)} <= cov["long_chain"].crossings for p in range(case("long_chain").P))
    assert any(count // SPAN < m // SPAN for _, count, m in cov["long_chain"].low_start)  # m in a later span than count
    assert sum(spans >= 4 for spans in cov["interleaved"].mixed.values()) >= 3  # roots with kept and dropped slots in every chunk of four spans
    for name in ("edge_N256", "edge_N512", "edge_N257", "long_chain"):
        c = case(name)
        assert any(c.move_slot[p] > 0 and not c.reset[p] and c.kept[p] > 1 for p in cov[name].full), name  # num_nodes == N
    chain = case("long_chain")
    assert chain.N == 3 * SPAN + 1 and sorted(int(m) for m in chain.move_slot[:5]) == [1, 255, 256, 257, 600]
    assert int(chain.move_slot[5]) == chain.tree["num_nodes"][5] - 1
    assert set(KINDS) - {"zero_visits", "proportional"} <= {k for name in CONSTRUCTED for k in case(name).kinds}
    return cov


def coverage_report():
    """The counts of `coverage` for every constructed shape, as lines of text (profiles/)."""
    lines = []
    for name, v in check_constructed().items():
        c = case(name)
        spans = sorted({span for _, span in v.below_kept})
        lines.append(f"{name}: P {c.P} N {c.N} C {c.C} num_nodes {v.num_nodes} moves {c.move_slot.tolist()} kept {c.kept}")
        lines.append(f"  parent below its span kept/not {len(v.below_kept)}/{v.below_dropped} (spans {spans}, roots {sorted({p for p, _ in v.below_kept})}); "
                     f"earlier chunk kept/not {v.earlier_kept}/{v.earlier_dropped}; same chunk {v.same_chunk}; longest in-chunk chain {v.longest}")
        lines.append(f"  kept links over 256/512 {sorted(v.crossings)}; pass 3 from count's chunk (root, count, m) {v.low_start}; full roots {v.full}; "
                     f"roots with kept and dropped slots in every chunk: spans {v.mixed}")
    return lines


WAYS =("one_launch", "two_launches", "given_move")


def ways(c, reset=True):
    """The three call sequences of a case, each from the case's tree: CHOOSE | REROOT in one call, CHOOSE and REROOT in two,
    REROOT alone with the caller's move_slot."""
    r = c.reset if reset else None
    return {"one_launch": [call(CHOOSE | REROOT, c.mode, reset=r)],
            "two_launches": [call(CHOOSE, c.mode), call(REROOT, reset=r)],
            "given_move": [call(REROOT, move_slot=c.move_slot, reset=r)]}


@functools.lru_cache(maxsize=None)
def modelled(name, way, reset=True):
    c = case(name)
    return run(c.tree, c.C, ways(c, reset)[way])


# ---- trees the caller has damaged -----------------------------------------------------------------------------------
DAMAGE_SHAPE = "G16_C16_P35"
DAMAGE = ("num_nodes_0", "num_nodes_N_plus_1", "move_slot_N", "move_slot_minus_2", "parent_self", "parent_N", "num_children_minus_1",
          "num_children_C_plus_5", "first_child_0", "first_child_n", "child_range_not_kept")


@functools.lru_cache(maxsize=None)
def damaged(name):
    """-> SimpleNamespace(case, p, m, seq, states, healthy): REROOT alone with the caller's moves, root p (with neighbours on
    both sides) moving to its most-visited child m, which has at least two children of its own, after the pokes of `name`;
    `healthy` is the same call without them."""
    c = case(DAMAGE_SHAPE)
    t, shp = c.tree, shapes(c.P, c.N, c.C)
    for p in range(1, c.P - 1):
        k, fc = int(t["num_children"][p, 0]), int(t["first_child"][p, 0])
        if k:
            m = fc + greedy_pick(t["visits"][p, fc:fc + k])
            if m != 1 and t["num_children"][p, m] >= 2:
                break
    else:
        raise AssertionError("no root suits")
    n = int(t["num_nodes"][p])
    move = c.move_slot.copy()
    move[p] = m
    reset = c.reset.copy()
    reset[p] = 0
    last_kept = subtree(t, p, m)[-1]
    poke = {"num_nodes_0": ("num_nodes", 0, p), "num_nodes_N_plus_1": ("num_nodes", c.N + 1, p), "move_slot_N": ("move_slot", c.N, p),
            "move_slot_minus_2": ("move_slot", -2, p), "parent_self": ("parent", n - 1, p, n - 1), "parent_N": ("parent", c.N, p, 2),
            "num_children_minus_1": ("num_children", -1, p, last_kept), "num_children_C_plus_5": ("num_children", c.C + 5, p, m),
            "first_child_0": ("first_child", 0, p, m), "first_child_n": ("first_child", n, p, m),
            "child_range_not_kept": ("first_child", 1, p, m)}[name]  # the root's own children: m's siblings are not kept
    f, value, *index = poke
    if f == "move_slot":  # the caller's move_slot is written after the pokes: an out-of-range move goes into that tensor itself
        move[p] = value
        pokes = ()
    else:
        pokes = ((f, flat(shp[f], *index), int(value)),)
    seq = [call(REROOT, move_slot=move, reset=reset, pokes=pokes)]
    healthy = run(t, c.C, [call(REROOT, move_slot=np.where(np.arange(c.P) == p, m, move).astype(np.int32), reset=reset)])
    return SimpleNamespace(case=c, p=p, m=m, n=n, seq=seq, pokes=pokes, move_slot=move, reset=reset, states=run(t, c.C, seq), healthy=healthy)


# ---- damage at depth: in the third span, after two spans have stored their ranks into remap --------------------------
DEEP_DAMAGE = ("parent_N", "parent_self", "first_child_n", "child_range_not_kept")
# shape: the root (with neighbours on both sides), its move, the kept slot of the third span whose parent is damaged, the kept
# node of that span whose child range is, and a child range of the right length that exists and is not kept
DEEP = {"long_chain": (2, 255, 600, 600, 1), "wide": (1, 5, 600, 513, 65)}
DEEP_CASES = [(shape, name) for shape in DEEP for name in DEEP_DAMAGE]


@functools.lru_cache(maxsize=None)
def damaged_deep(shape, name):
    """As `damaged`, in a constructed shape: REROOT alone with the caller's moves; the two neighbours of root p move to slot 0,
    the identity, so their trees stay as they are."""
    c = case(shape)
    p, m, s, node, elsewhere = DEEP[shape]
    t, shp, n = c.tree, shapes(c.P, c.N, c.C), int(c.tree["num_nodes"][p])
    move, reset = c.move_slot.copy(), c.reset.copy()
    move[p - 1:p + 2] = (0, m, 0)
    reset[p - 1:p + 2] = 0
    f, value, at = {"parent_N": ("parent", c.N, s), "parent_self": ("parent", s, s), "first_child_n": ("first_child", n, node),
                    "child_range_not_kept": ("first_child", elsewhere, node)}[name]
    pokes = ((f, flat(shp[f], p, at), int(value)),)
    seq = [call(REROOT, move_slot=move, reset=reset, pokes=pokes)]
    healthy = run(t, c.C, [call(REROOT, move_slot=move, reset=reset)])
    return SimpleNamespace(case=c, p=p, m=m, n=n, s=s, node=node, seq=seq, pokes=pokes, move_slot=move, reset=reset, states=run(t, c.C, seq), healthy=healthy)
