"""The cases of pcbenv_gumbel_advance (include/pcbenv_gumbel.h) and its CPU model: hand-built trees of every kind of root at
every group width, the calls made on them with scripted evaluations, and tools/gumbel_check.cpp -- csrc/pcb_gumbel.h as a
program of its own, built with AddressSanitizer and UBSan -- to run them.  tests/test_gumbel_model.py holds the model to the
specification (pcbenv/search.py:gumbel_select_root, gumbel_choose, gumbel_search), tests/test_gumbel_gpu.py the kernel to the
model.  Plain module, no test; needs no GPU.

A case is P roots of N slots, T = 3 levels, K = min(C, 3) candidates per evaluation.  Root p is of kind KINDS[p % len(KINDS)]:
  none   no children, evaluated once: the first ABSORB expands it      term   terminal at the root
  one    k = 1                                                         few    1 < k < Mc where there is such a k
  full   k = C, no visits below the root                               kept   k = C, the children hold visits and values
  flat   as kept, reward_hi == reward_lo                               zero   k = C, a zero prior and one above 1
The calls of a case:
  0        SELECT alone on counters the table presets per root: sim_index -- by p -- at 0, inside a phase, at a halving
           boundary, at n - 1, at n and above it; sim_visits all 7 on every other root, so that no child stands at the
           considered count ("S empty"), and 0 elsewhere
  1        ABSORB alone
  2        BEGIN | SELECT
  3 ..     n + 1 times ABSORB | SELECT: the scheduled simulations of the move, then PUCT descents from the root
  then     ABSORB alone, and CHOOSE
The evaluations are a hash of (case, call, root): values from {0.25, 0.5, 0.75}, K candidates mostly, priors from
puct_cases.PRIORS -- equal priors, hence equal PUCT scores below the root -- and now and then a terminal leaf.  N is small
enough for the larger roots to run out of slots: ERR_FULL.  ERR_TREE comes from the damage cases: the caller stores one
out-of-range value into root DAMAGE_ROOT before a call."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import model_harness as mh
import puct_cases as pc
from pcbenv.search import considered_visits

REPO = pc.REPO
BEGIN, ABSORB, SELECT, CHOOSE = 1, 2, 4, 8
ERR_FULL, ERR_TREE = 1, 2
FILL = -7
KINDS = ("kept", "none", "full", "term", "one", "zero", "few", "flat")
SEED = 0x67756D62656C5EED
BLOCK = 256
T = 3
TREE_FIELDS = pc.TREE_FIELDS
STATE_FIELDS = ("selected", "path_len", "paths") + TREE_FIELDS + ("sim_index", "sim_visits")
OUT_FIELDS = ("move_slot", "move_action", "child_weights", "child_policy", "child_actions", "root_value")
FLOATS = pc.FLOATS + ("root_value",)
POKED = ("selected", "num_nodes", "parent", "num_children", "first_child", "sim_index", "sim_visits")

# name: (C, P, Mc, n, c_visit, c_scale, first_root, step_index)
CASES = {
    "G4_C3_P131": (3, 131, 2, 4, 50.0, 1.0, 0, 77),            # three workgroups of 64 roots, the last partly filled
    "G4_C4_P131": (4, 131, 4, 8, 50.0, 0.1, 3, (1 << 32) + 5),  # a step index past 2^32
    "G8_C8_P67": (8, 67, 4, 5, 50.0, 1.0, 11, 77),
    "G16_C16_P67": (16, 67, 16, 6, 0.0, 1.0, 1000, (1 << 40) + 1),
    "G32_C20_P67": (20, 67, 8, 5, 50.0, 0.0, 2, 0),           # c_scale = 0: the target is the prior
    "G64_C64_P67": (64, 67, 64, 3, 25.0, 1.0, 0, 78),
}
DAMAGE_CASE, DAMAGE_ROOT = "G8_C8_P67", 16  # a root of kind "kept" with neighbours on either side
# name: (the call before which the poke is made, counted from the end where negative, tensor, value as a function of (N, k, C))
DAMAGE = {
    "sim_index_minus_1": (4, "sim_index", lambda N, k, C: -1),
    "sim_index_int_min": (4, "sim_index", lambda N, k, C: -(2 ** 31)),
    "sim_visits_int_max": (4, "sim_visits", lambda N, k, C: 2 ** 31 - 1),
    "select_more_children_than_C": (4, "num_children", lambda N, k, C: C + 1),
    "select_first_child_0": (4, "first_child", lambda N, k, C: 0),
    "select_first_child_past_the_end": (4, "first_child", lambda N, k, C: N - k + 1),
    "choose_children_int_max": (-1, "num_children", lambda N, k, C: 2 ** 31 - 1),
    "choose_first_child_negative": (-1, "first_child", lambda N, k, C: -(2 ** 31)),
    "choose_sim_visits_int_min": (-1, "sim_visits", lambda N, k, C: -(2 ** 31)),
    "absorb_selected_N": (4, "selected", lambda N, k, C: N),
    "absorb_num_nodes_0": (4, "num_nodes", lambda N, k, C: 0),
}

group_lanes = pc.group_lanes


def shapes(P, N, C, levels=T):
    s = pc.shapes(P, N, levels)
    s.update(sim_index=(P,), sim_visits=(P, C), move_slot=(P,), move_action=(P, 3), child_weights=(P, C), child_policy=(P, C),
             child_actions=(P, C, 3), root_value=(P,))
    return s


def program():
    """tools/gumbel_check.cpp as tests/model_harness.py:tool builds it; None without g++."""
    return mh.tool("gumbel_check")


def model_row(m, n):
    """csrc/pcb_gumbel.h:considered_row(m, n)."""
    return mh.run_words(program(), [np.array([1, m, n], np.int64)]).tolist()


def call(phases, evaluation=None, pokes=(), seed=SEED, step_index=77, first_root=0):
    return dict(phases=phases, evaluation=evaluation, pokes=tuple(pokes), seed=seed, step_index=step_index, first_root=first_root)


def run(state, C, K, n, Mc, rule, seq, levels=T):
    """state: dict of STATE_FIELDS (numpy) before the first call; rule: (c_puct, c_visit, c_scale).  -> [state after call i]:
    dicts of STATE_FIELDS and OUT_FIELDS (int64; FLOATS float64, child_policy float32) and `errors`, the error bits of that
    call.  A call may carry pokes, (tensor of POKED, flat index, value) stored into the state before its phases run.  Raises
    on anything on stderr.  levels: T, read off nothing: `paths` is [levels, P, 3]."""
    P, N = state["parent"].shape
    table = considered_visits(Mc, n).numpy()
    words = [np.array([0, P, N, C, levels, K, n, Mc, len(seq)] + [mh.bits(x) for x in rule], np.int64), table.astype(np.int64).ravel()]
    words += [mh.words(state[f], f in FLOATS) for f in STATE_FIELDS]
    for c in seq:
        words.append(np.array([c["phases"], mh.u64(c["seed"]), mh.u64(c["step_index"]), c["first_root"], len(c["pokes"])] +
                              [w for name, at, value in c["pokes"] for w in (POKED.index(name), at, value)], np.int64))
        if c["phases"] & ABSORB:
            value, over, count, actions, prior = c["evaluation"]
            assert actions.shape == (P, K, 3) and prior.shape == (P, K) and prior.dtype == np.float32
            words += [mh.words(value, True), mh.words(over), mh.words(count), mh.words(actions), mh.float32_words(prior)]
    return mh.cut(mh.run_words(program(), words), len(seq), STATE_FIELDS + OUT_FIELDS, shapes(P, N, C, levels), FLOATS, ("child_policy",))


def few_children(C, Mc, p):
    """k of a root of kind "few": 1 < k < Mc where there is such a k, else what fits."""
    return max(1, min(C, Mc - 1, 2 + p % 3)) if Mc > 2 else min(C, 2)


def preset_sim_index(p, n, table_row):
    """sim_index of root p before call 0: 0, inside a phase, at a halving boundary, n - 1, n, above n, by p."""
    boundary = next((t for t in range(1, n) if table_row[t] != table_row[t - 1]), n - 1)
    return (0, 1, boundary, n - 1, n, n + 3)[(p // 2) % 6]


def evaluation(name, i, P, K, kinds):
    """The scripted evaluation absorbed by call i of case `name`."""
    value, over, count = np.zeros(P), np.zeros(P, np.uint8), np.zeros(P, np.int32)
    actions, prior = np.zeros((P, K, 3), np.int32), np.zeros((P, K), np.float32)
    salt = sum(name.encode())
    for p in range(P):
        h = pc._mix(salt, i, p)
        value[p] = (0.25, 0.5, 0.75)[(h >> 16) % 3]
        over[p] = i >= 5 and (h >> 24) % 7 == 0
        count[p] = K if (h >> 40) % 4 else (h >> 32) % (K + 2)  # K + 1 among them: a count out of range is clamped
        for c in range(K):
            actions[p, c] = ((h + c) % 2, i, c)
            prior[p, c] = pc.PRIORS[pc._mix(h, c) % len(pc.PRIORS)]
    return value, over, count, actions, prior


@functools.lru_cache(maxsize=None)
def case(name):
    """-> SimpleNamespace(name, P, N, C, G, K, n, Mc, rule, kinds, k, state, seq, states): the tensors of CASES[name], its calls
    and the model's state after every call."""
    C, P, Mc, n, c_visit, c_scale, first_root, step_index = CASES[name]
    K = min(C, 3)
    N = 4 + C + 3 * K
    kinds = [KINDS[p % len(KINDS)] for p in range(P)]
    i32 = lambda shape, v: np.full(shape, v, np.int32)
    st = dict(selected=i32(P, FILL), path_len=i32(P, FILL), paths=i32((T, P, 3), FILL), num_nodes=i32(P, 1), parent=i32((P, N), -1),
              depth=i32((P, N), 0), visits=i32((P, N), 0), num_children=i32((P, N), 0), first_child=i32((P, N), -1),
              node_action=i32((P, N, 3), 0), prior=np.zeros((P, N)), value_sum=np.zeros((P, N)), value_max=np.full((P, N), -np.inf),
              terminal=np.zeros((P, N), np.uint8), reward_lo=np.full(P, 0.5), reward_hi=np.full(P, 0.5), sim_index=i32(P, 0), sim_visits=i32((P, C), 0))
    table = considered_visits(Mc, n).numpy()
    ks = np.zeros(P, np.int64)
    for p, kind in enumerate(kinds):
        k = {"none": 0, "term": 0, "one": 1, "few": few_children(C, Mc, p)}.get(kind, C)
        fc = 1 + p % 3 if k else -1
        ks[p] = k
        st["visits"][p, 0], st["value_sum"][p, 0], st["value_max"][p, 0] = 1, 0.5, 0.5
        st["terminal"][p, 0] = kind == "term"
        st["num_children"][p, 0], st["first_child"][p, 0], st["num_nodes"][p] = k, fc, fc + k if k else 1
        for c in range(k):
            s = fc + c
            st["parent"][p, s], st["depth"][p, s], st["node_action"][p, s] = 0, 1, (c % 2, p % 5, c)
            st["prior"][p, s] = pc.PRIORS[(p + c) % len(pc.PRIORS)]
            if kind in ("kept", "flat"):
                v = (3 * c + p) % 4
                mean = 0.5 if kind == "flat" else 0.25 + 0.25 * ((c + p) % 3)
                st["visits"][p, s], st["value_sum"][p, s], st["value_max"][p, s] = v, v * mean, mean if v else -np.inf
        if kind in ("kept", "flat"):
            below = st["visits"][p, fc:fc + k].sum()
            st["visits"][p, 0], st["value_sum"][p, 0] = 1 + below, 0.5 + st["value_sum"][p, fc:fc + k].sum()
        if kind == "kept":
            st["reward_lo"][p], st["reward_hi"][p], st["value_max"][p, 0] = 0.25, 0.75, 0.75
        if kind == "zero":
            st["prior"][p, fc], st["prior"][p, fc + k - 1] = 0.0, 1.5
        st["sim_index"][p] = preset_sim_index(p, n, table[min(Mc, k)])
        st["sim_visits"][p, :] = 7 if p % 2 else 0
    key = dict(seed=SEED, step_index=step_index, first_root=first_root)
    ev = lambda i: evaluation(name, i, P, K, kinds)
    seq = [call(SELECT, **key), call(ABSORB, ev(1), **key), call(BEGIN | SELECT, **key)]
    seq += [call(ABSORB | SELECT, ev(len(seq) + j), **key) for j in range(n + 1)]
    seq += [call(ABSORB, ev(len(seq)), **key), call(CHOOSE, **key)]
    rule = (1.25, c_visit, c_scale)
    return SimpleNamespace(name=name, P=P, N=N, C=C, G=group_lanes(C), K=K, n=n, Mc=Mc, rule=rule, kinds=kinds, k=ks, state=st, seq=seq,
                           states=run(st, C, K, n, Mc, rule, seq), first_root=first_root, step_index=step_index, table=table)


def before(c, i):
    """The state call i of case c starts from."""
    return c.state if i == 0 else c.states[i - 1]


def tree_of(state):
    """The tree of a model state as the dict the specification takes (torch, the integers as they are)."""
    t = {f: torch.from_numpy(np.array(state[f])) for f in TREE_FIELDS}
    t["node_action"] = t["node_action"].to(torch.int32)
    return t


@functools.lru_cache(maxsize=None)
def damaged(name):
    """-> (the case, the index of the damaged call, its sequence up to and including that call with the poke, the model's
    states of it, the root).  The calls after the damaged one are not made."""
    c = case(DAMAGE_CASE)
    p = DAMAGE_ROOT
    assert c.kinds[p] == "kept" and 0 < p < c.P - 1
    at, tensor, value = DAMAGE[name]
    at = at % len(c.seq)
    shp = shapes(c.P, c.N, c.C)
    k = int(before(c, at)["num_children"][p, 0])
    index = (p,) if len(shp[tensor]) == 1 else (p, 0)
    poke = (tensor, pc.flat(shp[tensor], *index), int(value(c.N, k, c.C)))
    seq = list(c.seq[:at]) + [dict(c.seq[at], pokes=(poke,))]
    return c, at, seq, run(c.state, c.C, c.K, c.n, c.Mc, c.rule, seq), p


@functools.lru_cache(maxsize=None)
def check_cases():
    """The table is what it is there for: every group width, roots across workgroups with a partly filled last group, every
    kind, and on the model's states every branch of the rule.  -> the cases."""
    cases = [case(name) for name in CASES]
    assert {c.G for c in cases} == {4, 8, 16, 32, 64} and all(c.P == (131 if c.G == 4 else 67) for c in cases)
    assert all(c.P > BLOCK // c.G and c.P % (BLOCK // c.G) for c in cases)
    assert any(c.step_index >> 32 for c in cases) and any(c.first_root for c in cases) and any(c.rule[2] == 0.0 for c in cases)
    seen = set()
    for c in cases:
        assert set(c.kinds) == set(KINDS)
        assert any(1 < c.k[p] < c.Mc for p in range(c.P) if c.kinds[p] == "few") or c.Mc <= 2
        for i, (q, st) in enumerate(zip(c.seq, c.states)):
            was = before(c, i)
            seen.update({1: "err_full", 2: "err_tree", 3: "err_full"}.get(st["errors"], "ok").split())
            if not q["phases"] & SELECT:
                continue
            for p in range(c.P):
                k, t = int(st["num_children"][p, 0]), int(0 if q["phases"] & BEGIN else was["sim_index"][p])
                if st["terminal"][p, 0] or k == 0:
                    seen.add("stops_at_root")
                    assert st["selected"][p] == 0 and st["path_len"][p] == 0 and (q["phases"] & BEGIN or st["sim_index"][p] == was["sim_index"][p])
                    continue
                if t >= c.n:
                    seen.add("puct_at_root")
                    assert st["sim_index"][p] == t
                    continue
                v = int(c.table[min(c.Mc, k), t])
                sims = np.zeros(c.C, np.int64) if q["phases"] & BEGIN else was["sim_visits"][p]
                seen.add("S_empty" if not (sims[:k] == v).any() else "S_part" if not (sims[:k] == v).all() else "S_all")
                seen.add("t_0" if t == 0 else "t_last" if t == c.n - 1 else "t_boundary" if c.table[min(c.Mc, k), t] != c.table[min(c.Mc, k), t - 1] else "t_inside")
                seen.add("k_below_Mc" if k < c.Mc else "k_above_Mc" if k > c.Mc else "k_is_Mc")
                assert st["sim_index"][p] == t + 1 and st["sim_visits"][p].sum() == sims.sum() + 1 and st["path_len"][p] >= 1
                if st["path_len"][p] >= 2:
                    seen.add("deeper")
                    # equal PUCT scores below the root: the node gone to has a sibling of the same prior, neither visited before
                    node, par = int(st["selected"][p]), int(st["parent"][p, st["selected"][p]])
                    if par > 0 and st["path_len"][p] == 2:
                        fc, kk = int(st["first_child"][p, par]), int(st["num_children"][p, par])
                        same = [s for s in range(fc, fc + kk) if s != node and st["prior"][p, s] == st["prior"][p, node] and
                                st["visits"][p, s] == 0 and st["visits"][p, node] == 0]
                        if same:
                            seen.add("tie_below")
                            assert node < min(same)
        last = c.states[-1]
        assert last["errors"] == 0 and (last["move_slot"][[p for p in range(c.P) if last["num_children"][p, 0] == 0]] == -1).all()
        seen.add("choose_without_children" if (last["move_slot"] == -1).any() else "")
    want = {"ok", "err_full", "stops_at_root", "puct_at_root", "S_empty", "S_part", "S_all", "t_0", "t_last", "t_boundary", "t_inside", "k_below_Mc",
            "k_above_Mc", "k_is_Mc", "deeper", "tie_below", "choose_without_children"}
    assert want <= seen, want - seen
    for name in DAMAGE:
        c, at, seq, states, p = damaged(name)
        if not name.startswith(("sim_visits", "choose_sim_visits")):
            assert states[-1]["errors"] & ERR_TREE, name
            seen.add("err_tree")
    assert "err_tree" in seen
    return cases


# ---- whole searches: the specification recorded, the model replaying it -------------------------------------------------
def init_state(P, N, C, levels):
    """What PCBENV_TREE_INIT leaves, the exchange tensors and the counters filled with FILL."""
    i32 = lambda shape, v: np.full(shape, v, np.int32)
    return dict(selected=i32(P, FILL), path_len=i32(P, FILL), paths=i32((levels, P, 3), FILL), num_nodes=i32(P, 1), parent=i32((P, N), -1),
                depth=i32((P, N), 0), visits=i32((P, N), 0), num_children=i32((P, N), 0), first_child=i32((P, N), -1),
                node_action=i32((P, N, 3), 0), prior=np.zeros((P, N)), value_sum=np.zeros((P, N)), value_max=np.full((P, N), -np.inf),
                terminal=np.zeros((P, N), np.uint8), reward_lo=np.full(P, np.inf), reward_hi=np.full(P, -np.inf), sim_index=i32(P, FILL),
                sim_visits=i32((P, C), FILL))


def state_of(tree, P, C, levels):
    """A tree of the specification (torch, `search_tree` or `puct_reroot`'s) as the state a replay starts from."""
    st = init_state(P, tree["parent"].shape[1], C, levels)
    for f in TREE_FIELDS:
        st[f] = tree[f].numpy().astype(st[f].dtype)
    return st


def record_search(P, levels, n, Mc, C, evaluate, rule, key, tree=None, capacity=None):
    """gumbel_search on the CPU -> (its result, the recorded evaluations as pc.record keeps them)."""
    from pcbenv.search import gumbel_search
    calls = []

    def recording(paths, path_len, s):
        ev = evaluate(paths, path_len, s)
        calls.append((paths.clone().numpy(), path_len.clone().numpy(), ev.value.to(torch.float64).numpy().copy(),
                      ev.terminal.to(torch.uint8).numpy().copy(), ev.cand_count.to(torch.int32).numpy().copy(),
                      ev.cand_actions.to(torch.int32).numpy().copy(), ev.cand_prior.to(torch.float32).numpy().copy()))
        return ev
    root = SimpleNamespace(num_envs=P, device="cpu", cfg=None)
    gs = gumbel_search(root, n, 100, recording, max_considered=Mc, c_visit=rule[1], c_scale=rule[2], c_puct=rule[0], max_children=C, max_steps=levels,
                       capacity=capacity, tree=tree, seed=key["seed"], first_root=key["first_root"], gumbel_step_index=key["step_index"])
    return gs, calls


def search_calls(calls, key):
    """The pcbenv_gumbel_advance calls of a recorded search: BEGIN | SELECT, ABSORB | SELECT per evaluation but the last,
    ABSORB, CHOOSE."""
    seq = [call(BEGIN | SELECT, **key)]
    seq += [call(ABSORB | (SELECT if m + 1 < len(calls) else 0), calls[m][2:], **key) for m in range(len(calls))]
    return seq + [call(CHOOSE, **key)]
