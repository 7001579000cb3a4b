"""The stream contract of the C ABI (include/pcbenv.h, "Streams"; tests/stream_cases.py is the table) on non-default
streams: every entry point runs on the stream it was given and on no other, the enqueue-only calls return before that
stream reaches them, the synchronous ones return after it has, a handle may move between streams behind the caller's own
events, and two handles on two streams share nothing.

Every test follows two rules.  (a) Stale input is valid input: every device buffer the library reads (actions, gather
index, reset mask, logits, bit rows, root index) exists and holds valid but wrong contents -- action (0, 0, 0), index
i -> i, mask 0, logits 0 -- before the side stream is delayed (stream_cases.lag); the true contents are written on the
side stream behind the delay.  A launch that went to another stream computes a wrong result from valid input and never
reads anything out of range.  (b) Results are read on the same side stream, behind the call.

Comparisons are bit for bit with a twin handle that made the same calls on the null stream without a delay, and with the
CPU oracle through the host model of tests/handle_model.py; the policy kernels keep the tolerances of
tests/test_sample_axis_gpu.py and tests/test_evaluate_axis_gpu.py against the float64 contract.

DRIVES names, per test, the functions of the table it drives; tests/test_stream_cases.py (no GPU) checks that every row
of the table is driven."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import evaluate_contract as ec
import factor_contract as fc
import handle_model as hm
import logits_cases as lc
from axis_cases import dense_of_bits, host_dist, legal_sets
from handle_model import SETUPS, Run, _bytes_equal, run_sequence
from pcbenv import _lib, named_config
from pcbenv.batched_env import FEATURE_KEYS, expand_compact_features
from pcbenv.config import KIND_PIN, KIND_SPATIAL
from stream_cases import ASYNC, LAG_MS, SYNC, lag, lagged, measured_lag_ms

pytestmark = pytest.mark.gpu

ENV_CALLS = ("pcbenv_reset", "pcbenv_step", "pcbenv_sample_actions", "pcbenv_step_sampled", "pcbenv_rollout_sampled",
             "pcbenv_gather", "pcbenv_playout", "pcbenv_sample_logits")
POLICY_CALLS = ("pcbenv_sample_logits", "pcbenv_sample_axis", "pcbenv_evaluate_logits", "pcbenv_evaluate_logits_backward",
                "pcbenv_evaluate_axis", "pcbenv_evaluate_axis_backward")
STEP_CALLS = ("pcbenv_reset", "pcbenv_step", "pcbenv_sample_actions", "pcbenv_step_sampled")
DRIVES = {
    "test_every_async_call_runs_on_the_stream_it_was_given": {
        "c3_b64": ENV_CALLS, "spatial10_slots4": ENV_CALLS, "c2_b48": ENV_CALLS, "policy_fp32": POLICY_CALLS, "policy_bf16": POLICY_CALLS},
    "test_async_calls_return_before_the_stream_reaches_them": ASYNC + SYNC,
    "test_call_sequences_on_a_lagging_side_stream": {
        name: ENV_CALLS + ("pcbenv_evaluate_logits", "pcbenv_get_state", "pcbenv_set_state")
        + (() if name == "c3_generator" else ("pcbenv_load_instances",)) for name in ("c3_generator", "c4_slots4_compact", "c3_both_t256")},
    "test_a_handle_may_move_between_streams": STEP_CALLS + ("pcbenv_get_state", "pcbenv_set_state", "pcbenv_instgen_device_enable",
                                                            "pcbenv_instgen_device_status"),
    "test_two_handles_on_two_streams": STEP_CALLS + ("pcbenv_gather", "pcbenv_load_instances"),
    "test_option_and_rebind_between_launches_on_a_side_stream": STEP_CALLS + ("pcbenv_load_instances",),
}

ENV_CASES = {
    # the pin kind with helpers and the terminal list live (default capacity B / 8), episodes staggered
    "c3_b64": (lambda: named_config("c3"), 64, {}),
    # the trajectory layout of the spatial kind: the feature cache and its tag, compact features, marginals
    "spatial10_slots4": (hm._small_spatial, 32, dict(num_slots=4, compact_features=True, mask_marginals=True)),
    "c2_b48": (lambda: named_config("c2"), 48, {}),
}


def _no_lag():
    pass


def _host(x):
    if isinstance(x, torch.Tensor):
        return x.cpu().numpy() if x.dtype != torch.bfloat16 else x.view(torch.int16).cpu().numpy()
    if isinstance(x, dict):
        return {k: _host(v) for k, v in x.items()}
    return x


def _same(a, b):
    """Two host snapshots, bit for bit (NaN included); returns the first key that differs, or None."""
    for k in a:
        if isinstance(a[k], dict):
            bad = _same(a[k], b[k])
            if bad is not None:
                return f"{k}/{bad}"
        elif isinstance(a[k], np.ndarray):
            if not _bytes_equal(a[k], b[k]):
                return k
        elif a[k] != b[k]:
            return k
    return None


def _snap(env, **extra):
    """Device-side copies, made on the current stream, of everything a call on the handle may write."""
    d = {"obs/" + k: v.clone() for k, v in env.traj.items()}
    if env.compact_features:  # the reference's float64 form, for the oracle
        d.update({"f64/" + k: v for k, v in expand_compact_features(env.cfg, {k: v for k, v in env.traj.items() if k in FEATURE_KEYS}).items()})
    d.update(reward=env.traj_reward.clone(), done=env.traj_done.clone(), info=env.traj_info.clone(), mask_bits=env.mask_bits())
    d.update({"marginal/" + k: v.clone() for k, v in env.traj_marginals.items()})
    d.update(extra)
    return d


def _unpacked(bits, cfg):
    """mask_bits() as the oracle's action_mask (handle_model.Driver.unpacked_mask_bits)."""
    cells = np.unpackbits(bits.view(np.uint8), axis=-1, bitorder="little")[..., :cfg.width]
    return np.ascontiguousarray(cells[:, [o & 1 for o in range(cfg.num_orientations)]])


def _check_oracle(model, cfg, snap, s, tag, expect=None, state_is_current=True):
    """Slot s of a host snapshot against the model: every observation tensor, reward and done of every slot, info of the
    transition `expect` = (reward, done, info) that has just written the slot, and the legal-mask bit rows."""
    ob = model.ob
    for key, v in snap.items():
        if not key.startswith("obs/"):
            continue
        k = key[4:]
        v = snap.get("f64/" + k, v)
        bad = ob.first_mismatch(k, v[s])
        assert bad < 0, (tag, k, "slot", s, "first row", bad)
    if expect is not None:
        rr, dd, ii = expect
        assert np.array_equal(snap["done"][s], dd), (tag, "done", np.flatnonzero(snap["done"][s] != dd)[:5].tolist())
        assert _bytes_equal(snap["reward"][s], rr), (tag, "reward")
        if cfg.kind in (KIND_PIN, KIND_SPATIAL):
            inf = snap["info"][s]
            has = ~np.isnan(inf[:, 0])
            assert _bytes_equal(inf[has], ii[has]), (tag, "info")
    if state_is_current:
        assert _bytes_equal(snap["reward"], model.R), (tag, "reward of some slot")
        assert np.array_equal(snap["done"], model.D), (tag, "done of some slot")
        bad = ob.first_mismatch("action_mask", _unpacked(snap["mask_bits"], cfg))
        assert bad < 0, (tag, "mask_bits", "first row", bad)
        if "marginal/rows" in snap:
            am = snap["obs/action_mask"][s].reshape(model.B, -1, cfg.height, cfg.width)
            assert np.array_equal(snap["marginal/rows"][s], am.max(axis=3)) and np.array_equal(snap["marginal/orientation"][s], am.max(axis=(2, 3))), tag


# ---------------------------------------------------------------------------------------------------------------
# every async call runs on the stream it was given
# ---------------------------------------------------------------------------------------------------------------
def _env_script(env, before, groups, seed=5):
    """Groups of eight calls made back to back on the current stream -- step, fused step, masked reset, gather, masked
    categorical draw, playout, two-step rollout, uniform draw -- with before() in front of each and a device-side copy of
    everything behind each; the host is not involved inside a group, so every call finds its predecessor still in flight.
    Returns the log [(call, slot written, arguments, copies)] with device tensors."""
    cfg, B, dev = env.cfg, env.num_envs, env.device
    rng = np.random.RandomState(seed)
    L, A = cfg.max_num_components, cfg.num_orientations * cfg.height * cfg.width
    stream = torch.cuda.current_stream(dev)
    i32 = dict(dtype=torch.int32, device=dev)
    acts, mask, idx = torch.zeros((B, 3), **i32), torch.zeros(B, dtype=torch.uint8, device=dev), torch.zeros(B, **i32)
    root, logits = torch.zeros(2 * B, **i32), torch.zeros((B, A), dtype=torch.float32, device=dev)
    ident = torch.arange(2 * B, **i32) % B
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt)
    sampled = env.sample_actions(0)
    log, t = [], 0
    for g in range(groups):
        # the true inputs of this group, staged on the device before anything is delayed
        bad = rng.rand(B) < 0.03
        true_acts = torch.where(up(bad, torch.bool)[:, None], up(rng.randint(-1, 70, size=(B, 3)), torch.int32), sampled)
        true_mask = up(np.arange(B) % L == g % L, torch.uint8)  # staggers the episodes
        gi = rng.randint(0, B, size=B)
        gi[rng.rand(B) < 0.1] = -1
        true_idx, true_root = up(gi, torch.int32), up(rng.randint(0, B, size=2 * B), torch.int32)
        true_logits = up(rng.randn(B, A) * 3.0, torch.float32)
        # rule (a): valid but wrong contents, complete before the delay
        acts.zero_(); mask.zero_(); logits.zero_()
        idx.copy_(ident[:B]); root.copy_(ident)
        stream.synchronize()

        env.select_slot(t + 1)
        before(); acts.copy_(true_acts); env.step(acts)
        log.append(("step", env.slot, dict(a=true_acts), _snap(env))); t += 1

        env.select_slot(t + 1)
        before(); fused = torch.zeros((B, 3), **i32); env.rollout_step(t, out=fused)
        log.append(("fused", env.slot, {}, _snap(env, a=fused))); t += 1

        before(); mask.copy_(true_mask); env.reset(mask)
        log.append(("reset", env.slot, dict(mask=true_mask), _snap(env)))

        before(); idx.copy_(true_idx); env.gather_(idx)
        log.append(("gather", env.slot, dict(idx=true_idx), _snap(env)))

        before(); logits.copy_(true_logits); drawn = env.sample_logits(logits, t)
        log.append(("sample_logits", env.slot, {}, dict(a=drawn[0], log_prob=drawn[1], entropy=drawn[2])))

        before(); root.copy_(true_root); po = env.playout(index=root, step_index=t)
        log.append(("playout", env.slot, {}, dict(reward=po.reward, done=po.done, length=po.length, actions=po.actions,
                                                  **({} if po.info is None else dict(info=po.info)))))

        env.select_slot(t + 1)
        before(); rec = torch.zeros((2, B, 3), **i32); env.rollout_steps(t, 2, out=rec)
        log.append(("rollout", env.slot, {}, _snap(env, rec=rec))); t += 2
        env.select_slot(env.slot + 1)  # the slot the last transition wrote

        before(); sampled = torch.zeros((B, 3), **i32); env.sample_actions(t, out=sampled)
        log.append(("sample_actions", env.slot, {}, dict(a=sampled)))
    stream.synchronize()
    return log


def _replay_on_model(run, log, tag):
    """The calls of a log (host copies) on the host model; step, reset, gather and the rollout against the oracle."""
    m, cfg, S = run.model, run.cfg, run.S
    for n, (call, s, args, snap) in enumerate(log):
        where = (tag, n, call)
        if call in ("step", "fused"):
            m.select(s)
            expect = m.step(args["a"] if call == "step" else snap["a"])
            _check_oracle(m, cfg, snap, s, where, expect)
        elif call == "reset":
            m.reset(args["mask"])
            _check_oracle(m, cfg, snap, s, where)
        elif call == "gather":
            m.gather(args["idx"])
            _check_oracle(m, cfg, snap, s, where)
        elif call == "rollout":
            m.select(s)
            for k in range(2):
                sk = (s + k) % S
                expect = m.step(snap["rec"][k], slot=sk, set_last_done=False)
                if k == 1 or S > 1:  # in place, the first transition's tensors have been overwritten
                    _check_oracle(m, cfg, snap, sk, where + (k,), expect, state_is_current=k == 1)
            m.select(s + 1)
        assert m.fresh_rows[m.slot].all()


POLICY_CASES = {"policy_fp32": torch.float32, "policy_bf16": torch.bfloat16}


@pytest.mark.parametrize("name", list(ENV_CASES) + list(POLICY_CASES))
def test_every_async_call_runs_on_the_stream_it_was_given(name):
    if name in POLICY_CASES:
        return _policy_case(POLICY_CASES[name])
    make_cfg, B, kw = ENV_CASES[name]
    cfg = make_cfg()
    groups = max(4, cfg.max_num_components // 2)  # four transitions per group: at least 2 x max_num_components
    make = lambda: Run(cfg, B, run_seed=3, queue_depth=3, auto_reset=True, **kw)
    twin = make()
    want = [(c, s, _host(a), _host(d)) for c, s, a, d in _env_script(twin.env, _no_lag, groups)]
    twin.close()
    side = torch.cuda.Stream()
    with lagged(side) as before:
        run = make()
        t0 = time.perf_counter()
        got = [(c, s, _host(a), _host(d)) for c, s, a, d in _env_script(run.env, before, groups)]  # read on the side stream
        print(f"STREAMS {name} B={B} groups={groups} lags={before.calls} wall={time.perf_counter() - t0:.2f}s")
        assert before.calls == 8 * groups
        for n, (w, g) in enumerate(zip(want, got)):
            assert w[:2] == g[:2]
            bad = _same(w[2], g[2]) or _same(w[3], g[3])
            assert bad is None, (name, "call", n, w[0], "differs from the null-stream twin in", bad)
        _replay_on_model(run, got, name)
        run.close()


def _policy_script(env, before, dtype, seed=9):
    """The six policy entry points back to back on the current stream: the draws on the handle's B environments, the
    evaluate calls on 257 rows of the caller's own; every input stale until its delay has passed."""
    cfg, B, dev, N = env.cfg, env.num_envs, env.device, 257
    O, H, W = cfg.num_orientations, cfg.height, cfg.width
    A, WW = O * H * W, (W + 63) // 64
    rng = np.random.RandomState(seed)
    stream = torch.cuda.current_stream(dev)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt).contiguous()
    for t in range(3):  # a few placements, so that the legal sets are not the empty board's
        env.step(env.sample_actions(t))
    bits_env = env.mask_bits().cpu().numpy()
    dense_env = dense_of_bits(bits_env, cfg)
    # true inputs
    classes = lc.bits(cfg.kind, O, H, W, rng)
    rows_bits = classes[rng.randint(len(classes), size=N)]
    dense = dense_of_bits(rows_bits, cfg)
    legal = dense.reshape(N, A)
    l_flat = lc.tame(rng, legal)
    a_flat = lc.stored_actions(rng, legal, l_flat).astype(np.int32)
    a_tuple = np.stack([a_flat // (H * W), a_flat % (H * W) // W, a_flat % W], axis=1).astype(np.int32)
    axis, given = 1, (0,)  # p(x | o)
    Lx, ok = legal_sets(dense, axis, given, a_tuple)
    l_axis = lc.tame(rng, Lx)
    g_lp, g_h = rng.randn(N).astype(np.float32), (0.01 * rng.randn(N)).astype(np.float32)
    env_logits = lc.tame(rng, dense_env.reshape(B, A))
    # (no -inf here: a stage's legal set depends on what the stage before drew, and it must keep a finite logit)
    stage_logits = [lc.tame(rng, np.ones((B, n), bool), p_neg_inf=0.0) for n in (O, H, W)]
    true = dict(logits=up(l_flat, dtype), bits=up(rows_bits, torch.int64), a_flat=up(a_flat, torch.int32), a_tuple=up(a_tuple, torch.int32),
                l_axis=up(l_axis, dtype), g_lp=up(g_lp, torch.float32), g_h=up(g_h, torch.float32), env_logits=up(env_logits, dtype),
                stage=[up(x, dtype) for x in stage_logits])
    buf = {k: torch.zeros_like(v) for k, v in true.items() if k != "stage"}  # logits 0, no legal bit, action (0, 0, 0), gradients 0
    buf["stage"] = [torch.zeros_like(v) for v in true["stage"]]
    stream.synchronize()
    out = {}

    def fill(*names):
        for k in names:
            buf[k].copy_(true[k])

    before(); fill("env_logits"); a, lp, ent = env.sample_logits(buf["env_logits"], 3)
    out["sample_logits"] = dict(a=a, log_prob=lp, entropy=ent)
    drawn = torch.zeros((B, 3), dtype=torch.int32, device=dev)
    for ax, giv in ((0, ()), (1, (0,)), (2, (0, 1))):  # p(o) p(x|o) p(y|o,x): every stage reads what the one before drew
        before(); buf["stage"][ax].copy_(true["stage"][ax]); lp, ent = env.sample_axis(ax, buf["stage"][ax], 3, drawn, giv)
        out[f"sample_axis{ax}"] = dict(a=drawn.clone(), log_prob=lp, entropy=ent)
    stats = torch.zeros((N, 4), dtype=torch.float32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    before(); fill("logits", "bits", "a_flat"); lp, ent = env.evaluate_logits_forward(buf["logits"], buf["bits"], buf["a_flat"], stats, err)
    out["evaluate_logits"] = dict(log_prob=lp, entropy=ent, stats=stats.clone(), err=err.clone())
    before(); fill("g_lp", "g_h")  # stats: still in flight
    grad = env.evaluate_logits_backward(buf["logits"], buf["bits"], buf["a_flat"], stats, buf["g_lp"], buf["g_h"])
    out["evaluate_logits_backward"] = dict(grad=grad)
    err2 = torch.zeros(1, dtype=torch.int32, device=dev)
    before(); fill("l_axis", "a_tuple"); lp, ent = env.evaluate_axis_forward(axis, given, buf["l_axis"], buf["bits"], buf["a_tuple"], err2)
    out["evaluate_axis"] = dict(log_prob=lp, entropy=ent, err=err2.clone())
    before(); gax = env.evaluate_axis_backward(axis, given, buf["l_axis"], buf["bits"], buf["a_tuple"], buf["g_lp"], buf["g_h"])
    out["evaluate_axis_backward"] = dict(grad=gax)
    stream.synchronize()
    read = lambda x: x.float().cpu().numpy().astype(np.float64)  # what the kernels read from the logits' dtype
    host = dict(dense_env=dense_env, legal=legal, a_flat=a_flat, a_tuple=a_tuple, Lx=Lx, ok=ok, axis=axis, given=given,
                g_lp=g_lp.astype(np.float64), g_h=g_h.astype(np.float64), l_flat=read(true["logits"]), l_axis=read(true["l_axis"]),
                env_logits=read(true["env_logits"]), stage=[read(x) for x in true["stage"]])
    return out, host


def _bf16_round(x):
    return torch.from_numpy(np.asarray(x, np.float64)).to(torch.bfloat16).double().numpy()


def _bf16_ulp(x):
    ax = np.abs(x)
    with np.errstate(divide="ignore"):
        return np.where(ax > 0, 2.0 ** (np.floor(np.log2(np.where(ax > 0, ax, 1.0))) - 7), 0.0)


def _check_policy_contract(cfg, out, h, dtype):
    """The side stream's results against the float64 contract, with the tolerances of tests/test_sample_axis_gpu.py and
    tests/test_evaluate_axis_gpu.py: atol 1e-4 on log_prob and entropy; gradients within 4 x e_ref + 1e-7 (bf16: of the
    contract rounded to bf16, plus one bf16 ulp), e_ref the error of torch's float32 chain on the CPU."""
    O, H, W = cfg.num_orientations, cfg.height, cfg.width
    B = len(h["dense_env"])
    rows = np.arange(B)
    f = lambda x: np.asarray(x, np.float64) if x.dtype != np.int16 else torch.from_numpy(x).view(torch.bfloat16).double().numpy()
    # the draws: legal, and log_prob / entropy of the drawn value
    legal_env = h["dense_env"].reshape(B, -1)
    a = out["sample_logits"]["a"]
    flat = a[:, 0] * H * W + a[:, 1] * W + a[:, 2]
    has = legal_env.any(1)
    assert legal_env[has, flat[has]].all()
    M, Z, _, ent = host_dist(h["env_logits"], legal_env)
    np.testing.assert_allclose(out["sample_logits"]["log_prob"][has], (h["env_logits"][rows, flat] - M - np.log(Z))[has], atol=1e-4, rtol=0)
    np.testing.assert_allclose(out["sample_logits"]["entropy"][has], ent[has], atol=1e-4, rtol=0)
    acts = np.zeros((B, 3), np.int32)
    for ax, giv in ((0, ()), (1, (0,)), (2, (0, 1))):
        L, ok = legal_sets(h["dense_env"], ax, giv, acts)
        acts = out[f"sample_axis{ax}"]["a"]
        v, has = acts[:, ax], L.any(1)
        assert ok.all() and L[has, v[has]].all() and (v[~has] == 0).all(), ax
        l = h["stage"][ax]
        M, Z, _, ent = host_dist(l, L)
        np.testing.assert_allclose(out[f"sample_axis{ax}"]["log_prob"][has], (l[rows, v] - M - np.log(Z))[has], atol=1e-4, rtol=0)
        np.testing.assert_allclose(out[f"sample_axis{ax}"]["entropy"][has], ent[has], atol=1e-4, rtol=0)
    # the evaluate calls
    N = len(h["legal"])
    z = np.zeros(N)

    def grad_ok(got, want, l, L, a, a_in, what):
        _, _, ref, fin = lc.chain32(l, L, np.where(a_in, a, 0), h["g_lp"], h["g_h"])
        use = a_in & fin
        e_ref = float(np.abs(ref - want)[use].max()) if use.any() else 0.0
        bound = 4.0 * e_ref + 1e-7
        target, allow = (want, bound) if dtype == torch.float32 else (_bf16_round(want), bound + _bf16_ulp(_bf16_round(want)))
        e_k = float(np.abs(got - target).max())
        print(f"STREAMS-GRAD {what} {dtype} ref_f32_chain_err {e_ref:.3e} kernel_err {e_k:.3e} bound {bound:.3e}")
        assert (np.abs(got - target) <= allow).all(), (what, dtype, e_k, bound)

    lp, ent, bits, _ = ec.evaluate(h["l_flat"], h["legal"], h["a_flat"])
    assert int(out["evaluate_logits"]["err"][0]) == bits
    np.testing.assert_allclose(out["evaluate_logits"]["log_prob"], lp, atol=1e-4, rtol=0)
    np.testing.assert_allclose(out["evaluate_logits"]["entropy"], ent, atol=1e-4, rtol=0)
    a = h["a_flat"].astype(np.int64)
    a_in = h["legal"].any(1) & h["legal"][np.arange(N), a]
    grad_ok(f(out["evaluate_logits_backward"]["grad"]), ec.gradient(h["l_flat"], h["legal"], a, h["g_lp"], h["g_h"]), h["l_flat"], h["legal"], a, a_in,
            "evaluate_logits_backward")
    ax, L, l = h["axis"], h["Lx"], h["l_axis"]
    a = h["a_tuple"][:, ax].astype(np.int64)
    rows_c = [fc.evaluate(l[r], L[r], h["ok"][r], a[r]) for r in range(N)]
    bits = 0
    for _, _, b in rows_c:
        bits |= b
    assert int(out["evaluate_axis"]["err"][0]) == bits
    np.testing.assert_allclose(out["evaluate_axis"]["log_prob"], np.array([x[0] for x in rows_c]), atol=1e-4, rtol=0)
    np.testing.assert_allclose(out["evaluate_axis"]["entropy"], np.array([x[1] for x in rows_c]), atol=1e-4, rtol=0)
    want = np.stack([fc.gradient(l[r], L[r], a[r], h["g_lp"][r], h["g_h"][r]) for r in range(N)])
    a_in = L.any(1) & L[np.arange(N), a]
    grad_ok(f(out["evaluate_axis_backward"]["grad"]), want, l, L, a, a_in, "evaluate_axis_backward")


def _policy_case(dtype):
    cfg, B = named_config("c3"), 64
    make = lambda: Run(cfg, B, run_seed=3, queue_depth=3, auto_reset=True)
    twin = make()
    want, _ = _policy_script(twin.env, _no_lag, dtype)
    want = _host(want)
    twin.close()
    side = torch.cuda.Stream()
    with lagged(side) as before:
        run = make()
        got, host = _policy_script(run.env, before, dtype)
        got = _host(got)  # read on the side stream
        assert before.calls == 8
        bad = _same(want, got)
        assert bad is None, ("differs from the null-stream twin in", bad)
        _check_policy_contract(cfg, got, host, dtype)
        run.close()


# ---------------------------------------------------------------------------------------------------------------
# async calls return early, sync calls return late
# ---------------------------------------------------------------------------------------------------------------
def _async_calls(env, N=257):
    """name -> a closure making that call on the current stream with valid arguments (values do not matter here)."""
    cfg, B, dev = env.cfg, env.num_envs, env.device
    O, H, W = cfg.num_orientations, cfg.height, cfg.width
    A, WW = O * H * W, (W + 63) // 64
    i32 = dict(dtype=torch.int32, device=dev)
    acts, out3, idx = torch.zeros((B, 3), **i32), torch.zeros((B, 3), **i32), torch.arange(B, **i32)
    mask = torch.ones(B, dtype=torch.uint8, device=dev)
    rec = torch.zeros((2, B, 3), **i32)
    logits, rows_logits = torch.zeros((B, A), device=dev), torch.zeros((N, A), device=dev)
    bits = torch.full((N, 2, H, WW), -1, dtype=torch.int64, device=dev)
    ra, rt = torch.zeros(N, **i32), torch.zeros((N, 3), **i32)
    stats, g = torch.zeros((N, 4), device=dev), torch.ones(N, device=dev)
    lx, ly = torch.zeros((B, H), device=dev), torch.zeros((N, W), device=dev)
    bad = torch.full((B, 3), -1, **i32)  # no such action: every episode ends, every step consumes an instance
    t = [0]

    def nxt():
        t[0] += 1
        return t[0]
    return {
        "pcbenv_reset": lambda: env.reset(mask),
        "pcbenv_step": lambda: env.step(bad),
        "pcbenv_sample_actions": lambda: env.sample_actions(nxt(), out=out3),
        "pcbenv_step_sampled": lambda: env.rollout_step(nxt(), out=out3),
        "pcbenv_rollout_sampled": lambda: env.rollout_steps(nxt(), 2, out=rec),
        "pcbenv_gather": lambda: env.gather_(idx),
        "pcbenv_playout": lambda: env.playout(index=idx, step_index=nxt(), max_steps=2),
        "pcbenv_sample_logits": lambda: env.sample_logits(logits, nxt()),
        "pcbenv_evaluate_logits": lambda: env.evaluate_logits_forward(rows_logits, bits, ra, stats),
        "pcbenv_evaluate_logits_backward": lambda: env.evaluate_logits_backward(rows_logits, bits, ra, stats, g, g),
        "pcbenv_sample_axis": lambda: env.sample_axis(1, lx, nxt(), acts, (0,)),
        "pcbenv_evaluate_axis": lambda: env.evaluate_axis_forward(2, (0, 1), ly, bits, rt),
        "pcbenv_evaluate_axis_backward": lambda: env.evaluate_axis_backward(2, (0, 1), ly, bits, rt, g, g),
    }


def gen_protocol_counts(consumes, Q):
    """The fills started and the fill waits the host protocol of csrc/pcb_gen.hip makes for a sequence of launches that may
    consume `consumes[i]` records per environment, from a quiescent queue of depth Q (a restatement of gen_before_launch /
    gen_after_launch: the library keeps these counters on the host and exports none of them)."""
    fills = waits = 0
    waited = outstanding_since = 0
    outstanding = False
    for n in consumes:
        if waited + n > Q:
            if not outstanding:
                fills += 1
                outstanding_since = 0
            waits += 1
            waited, outstanding = outstanding_since, False
            if waited + n > Q:
                fills += 1
                waits += 1
                waited = 0
        waited += n
        if outstanding:
            outstanding_since += n
        elif waited * 2 >= Q:
            fills += 1
            outstanding, outstanding_since = True, 0
    return fills, waits


def test_async_calls_return_before_the_stream_reaches_them():
    cfg, B, Q = named_config("c3"), 64, 3
    side = torch.cuda.Stream()
    host_ms = {}
    with lagged(side) as before:
        print(f"STREAMS lag asked {LAG_MS:.1f} ms measured {measured_lag_ms(side):.2f} ms")

        def early(name, call):
            before()
            reached = torch.cuda.Event()  # completes when the stream has passed the delay and gets to the call
            reached.record(side)
            t0 = time.perf_counter()
            call()
            dt = 1e3 * (time.perf_counter() - t0)
            ev = torch.cuda.Event()
            ev.record(side)
            # (the second alone would not do: behind a call that waited for the stream, `ev` is recorded on an idle stream
            # and may or may not have completed a microsecond later)
            assert not reached.query(), f"{name} returned only after the stream had passed a {LAG_MS} ms delay ({dt:.2f} ms on the host)"
            assert not ev.query(), name
            host_ms[name] = max(host_ms.get(name, 0.0), dt)

        # a host-fed handle: every async row once, each behind its own delay
        run = Run(cfg, B, run_seed=3, queue_depth=Q, auto_reset=True)
        calls = _async_calls(run.env)
        assert set(calls) == set(ASYNC)
        for name in ASYNC:
            calls[name]()  # once without a delay: kernels loaded, buffers of the wrappers allocated
        side.synchronize()
        for name in ASYNC:
            early(name, calls[name])
        side.synchronize()
        # the sync rows: an event recorded behind a delay, before the call, has completed when the call returns
        env = run.env
        packed = env._native.next_packed()
        nbytes = env._L.pcbenv_state_bytes(env._h)
        blob = np.empty(nbytes, np.uint8)
        lo, hi, err = C.c_uint32(), C.c_uint32(), C.c_uint32()
        inst = np.empty_like(packed)
        gen = Run(cfg, B, run_seed=4, queue_depth=Q, auto_reset=True)  # the generator is enabled below, behind a delay
        seeds = np.ascontiguousarray([hm.env_seed(4, i) for i in range(B)], np.uint32)

        def late(name, call):
            before()
            ev = torch.cuda.Event()
            ev.record(side)
            rc = call()
            assert ev.query(), f"{name} returned before the stream had done what was enqueued in front of it"
            assert rc == 0, (name, rc)

        s = env._stream
        late("pcbenv_load_instances", lambda: env._L.pcbenv_load_instances(env._h, None, B, 1, packed.ctypes.data, s()))
        late("pcbenv_get_state", lambda: env._L.pcbenv_get_state(env._h, blob.ctypes.data, s()))
        late("pcbenv_set_state", lambda: env._L.pcbenv_set_state(env._h, blob.ctypes.data, s()))
        late("pcbenv_get_instances", lambda: env._L.pcbenv_get_instances(env._h, 0, inst.ctypes.data, s()))
        late("pcbenv_queue_cursors", lambda: env._L.pcbenv_queue_cursors(env._h, C.byref(lo), C.byref(hi), s()))
        run.close()
        g = gen.env
        late("pcbenv_instgen_device_enable", lambda: g._L.pcbenv_instgen_device_enable(g._h, seeds.ctypes.data, g._stream()))
        g.device_instances = True
        late("pcbenv_instgen_device_status", lambda: g._L.pcbenv_instgen_device_status(g._h, C.byref(err), g._stream()))
        assert err.value == 0
        # with the generator on: 3 x queue_depth steps and more, every one of which ends every episode and so consumes a
        # record per environment -- refills and waits for a fill are part of these calls, and they must return early too
        calls = _async_calls(g)
        consumes = []
        for k in range(4 * Q):
            name = ("pcbenv_step", "pcbenv_step_sampled", "pcbenv_step", "pcbenv_rollout_sampled", "pcbenv_step", "pcbenv_reset")[k % 6]
            early(name + " (generator)", calls[name])
            consumes.append(2 if name == "pcbenv_rollout_sampled" else 1)
        fills, waits = gen_protocol_counts(consumes, Q)
        lo, hi = g.queue_cursors()
        print(f"STREAMS generator queue_depth={Q} launches={len(consumes)} records/env={sum(consumes)} fills={fills} waits={waits} cursors=({lo}, {hi})")
        assert fills >= 3 and waits >= 3
        assert hi > 2 * Q, "the episodes did not end often enough to go round the queue"
        assert g.device_instance_errors() == 0
        gen.close()
    slow = max(host_ms, key=host_ms.get)
    print("STREAMS host ms per async call (behind a delay): " + " ".join(f"{k}={v:.3f}" for k, v in sorted(host_ms.items())))
    print(f"STREAMS slowest async call on the host: {slow} {host_ms[slow]:.3f} ms; the delay is {LAG_MS / host_ms[slow]:.0f} x that")


# ---------------------------------------------------------------------------------------------------------------
# call sequences on a lagging side stream
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c3_generator", "c4_slots4_compact", "c3_both_t256"])
def test_call_sequences_on_a_lagging_side_stream(name):
    setup = SETUPS[name]
    side = torch.cuda.Stream()
    with lagged(side) as before:
        counts = run_sequence(setup, setup.seeds[0], before_op=lambda i, op: before())
    assert before.calls == setup.length
    if setup.replay:
        assert counts["capture"] == 1 and counts["replay"] >= 1
    print(f"STREAMS-SEQ {name} ops={sum(counts.values())} lags={before.calls} " + " ".join(f"{k}={v}" for k, v in sorted(counts.items())))


# ---------------------------------------------------------------------------------------------------------------
# a handle moves between streams; two handles on two streams
# ---------------------------------------------------------------------------------------------------------------
def _step_on(env, t, fused):
    """One transition on the current stream, no host in it; returns device copies of what it wrote and the actions."""
    if fused:
        a = torch.zeros((env.num_envs, 3), dtype=torch.int32, device=env.device)
        env.rollout_step(t, out=a)
    else:
        a = env.sample_actions(t)
        env.step(a)
    return _snap(env, a=a)


def _check_steps(run, snaps, tag):
    """Host copies of _step_on's results, in order, against the model."""
    for t, snap in enumerate(snaps):
        expect = run.model.step(snap["a"])
        _check_oracle(run.model, run.cfg, snap, 0, (tag, "step", t), expect)


def test_a_handle_may_move_between_streams():
    cfg, B, Q = named_config("c3"), 64, 3
    steps = 3 * cfg.max_num_components  # 3 episodes (the placements of an episode never outnumber the components)
    make = lambda: Run(cfg, B, run_seed=5, queue_depth=Q, auto_reset=True, device_instances=True)

    def play(run, streams, delay, prev):
        """prev: the stream the handle was created and reset on."""
        env, snaps = run.env, []
        save_at = steps // 2 + 1  # an odd step
        for t in range(steps):
            cur = streams[t % 2]
            with torch.cuda.stream(cur):
                if prev is not cur:
                    cur.wait_stream(prev)  # the caller's own event: everything below is ordered behind the step before
                if t == save_at + 1:  # restored on the other stream than the one the checkpoint was taken on
                    env.load_state_dict(sd)
                snaps.append(_step_on(env, t, fused=t % 3 == 0))
                if t == save_at:
                    sd = env.state_dict()
                delay(cur)  # on the stream that is about to be left
            prev = cur
        for s in set(streams):
            s.synchronize()
        with torch.cuda.stream(streams[0]):
            errors = env.device_instance_errors()
            cursors = env.queue_cursors()
        return [_host(s) for s in snaps], errors, cursors

    null = torch.cuda.current_stream()
    twin = make()
    want, errors, cursors = play(twin, (null, null), lambda s: None, null)
    twin.close()
    assert errors == 0
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        run = make()  # created, enabled and reset on S1
    got, errors, moved_cursors = play(run, (s2, s1), lambda s: lag(s), s1)  # odd steps on S1, even steps on S2
    assert errors == 0, "a reset found its record missing, or a stream stopped"
    assert moved_cursors == cursors and cursors[1] > Q
    for t, (w, g) in enumerate(zip(want, got)):
        bad = _same(w, g)
        assert bad is None, ("step", t, "differs from the null-stream twin in", bad)
    _check_steps(run, got, "moved")
    with torch.cuda.stream(s1):
        run.close()
    print(f"STREAMS-MOVE steps={steps} cursors={cursors}")


def test_two_handles_on_two_streams():
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    c3, c2 = named_config("c3"), named_config("c2")
    with torch.cuda.stream(s1):
        a = Run(c3, 64, run_seed=3, queue_depth=3, auto_reset=True)
    with torch.cuda.stream(s2):
        b = Run(c2, 48, run_seed=4, queue_depth=3, auto_reset=True)
    snaps_a, snaps_b = [], []
    for t in range(2 * c3.max_num_components):  # 2 episodes of the longer kind; neither stream waits for the other
        with torch.cuda.stream(s1):
            if t % 2 == 0:
                lag(s1)
            snaps_a.append(_step_on(a.env, t, fused=t % 3 == 1))
        with torch.cuda.stream(s2):
            if t % 2 == 1:
                lag(s2)
            snaps_b.append(_step_on(b.env, t, fused=t % 3 == 2))
    with torch.cuda.stream(s1):
        snaps_a = [_host(s) for s in snaps_a]
    with torch.cuda.stream(s2):
        snaps_b = [_host(s) for s in snaps_b]
        b.close()
    _check_steps(a, snaps_a, "c3 on S1")
    _check_steps(b, snaps_b, "c2 on S2")
    # a gather across two handles: the source's last step is still behind a delay on S1 when the gather arrives on S2,
    # ordered behind it by the caller's event alone
    with torch.cuda.stream(s2):
        d = Run(c3, 32, run_seed=6, queue_depth=3, auto_reset=True)
        idx = torch.arange(32, dtype=torch.int32, device=d.env.device)  # rule (a): i -> i is valid for a source of 64
        true_idx = torch.from_numpy(np.random.RandomState(2).randint(-1, 64, size=32).astype(np.int32)).to(d.env.device)
        s2.synchronize()
    with torch.cuda.stream(s1):
        lag(s1)
        last = _step_on(a.env, 2 * c3.max_num_components, fused=False)
        ev = torch.cuda.Event()
        ev.record(s1)
    with torch.cuda.stream(s2):
        lag(s2)
        idx.copy_(true_idx)
        s2.wait_event(ev)
        d.env.gather_(idx, source=a.env)
        after = _host(_snap(d.env))
    with torch.cuda.stream(s1):
        last = _host(last)
    _check_oracle(a.model, c3, last, 0, "source's last step", a.model.step(last["a"]))
    d.model.gather(true_idx.cpu().numpy(), a.model)
    _check_oracle(d.model, c3, after, 0, "gather across handles")
    # the message of one handle stays when the other refuses a call
    L = a.env._L
    with pytest.raises(ValueError):
        d.env.set_option("terminal_teams", -1)
    mine = L.pcbenv_last_error(d.env._h)
    assert b"terminal-list" in mine
    with pytest.raises(ValueError):
        a.env.set_option("gen_lanes", 48)
    assert L.pcbenv_last_error(d.env._h) == mine and b"lanes" in L.pcbenv_last_error(a.env._h)
    with torch.cuda.stream(s2):
        d.close()
    with torch.cuda.stream(s1):
        a.close()


# ---------------------------------------------------------------------------------------------------------------
# pcbenv_set_option and pcbenv_bind_buffers_slots between launches on a side stream
# ---------------------------------------------------------------------------------------------------------------
def _delayed_step(run, t, before, acts, true_acts, rng, p_bad=0.01):
    """One explicit step behind a delay, the actions stale until the delay has passed; returns the actions.  The model is
    stepped and compared by _settle, after whatever the test does while the step is in flight."""
    env, B = run.env, run.B
    a = env.sample_actions(t).cpu().numpy()
    bad = rng.rand(B) < p_bad
    a[bad] = rng.randint(-1, 70, size=(int(bad.sum()), 3))
    true_acts.copy_(torch.from_numpy(a))
    acts.zero_()
    torch.cuda.current_stream().synchronize()
    before(); acts.copy_(true_acts); env.step(acts)
    return a


def _settle(run, a, tag, obs=None):
    """The model takes the transition; reward, done, info and every tensor (of `obs`: a slot's tensors held by the caller,
    default the handle's selected slot) against the oracle, read on the current stream."""
    env, cfg = run.env, run.cfg
    rr, dd, ii = run.model.step(a)
    r, d, inf = (env.reward, env.done, env.info_raw) if obs is None else obs[1]
    assert np.array_equal(d.cpu().numpy(), dd), (tag, "done")
    assert _bytes_equal(r.cpu().numpy(), rr), (tag, "reward")
    inf = inf.cpu().numpy()
    has = ~np.isnan(inf[:, 0])
    assert _bytes_equal(inf[has], ii[has]), (tag, "info")
    run.model.I[run.model.slot] = inf
    if obs is None:
        run.compare_oracle(tag)
    else:
        for k, v in obs[0].items():
            bad = run.ob.first_mismatch(k, v.cpu().numpy())
            assert bad < 0, (tag, k, bad)


def test_option_and_rebind_between_launches_on_a_side_stream():
    side = torch.cuda.Stream()
    rng = np.random.RandomState(8)
    with lagged(side) as before:
        # the terminal list's capacity changes while a delay and a step are in flight on the side stream
        cfg, B = named_config("c3"), 512
        L = cfg.max_num_components
        run = Run(cfg, B, run_seed=3, queue_depth=3, auto_reset=True)
        env = run.env
        acts, true_acts = (torch.zeros((B, 3), dtype=torch.int32, device=env.device) for _ in range(2))
        values = (0, 16, 64, B // 8)
        for t in range(2 * L):
            a = _delayed_step(run, t, before, acts, true_acts, rng)
            if t % 2 == 0:
                env.set_option("terminal_teams", values[(t // 2) % 4])
            _settle(run, a, ("option", t))
            if t < L:  # stagger: from here on 1 / L of the batch ends an episode in every launch
                m = (np.arange(B) % L == t).astype(np.uint8)
                env.reset(torch.from_numpy(m))
                run.model.reset(m)
        run.close()
        # the spatial trajectory layout (feature cache and tags) is bound to a fresh set of tensors in the middle of an
        # episode, while a delay and a step into the old set are in flight
        cfg, B = hm._small_spatial(), 32
        run = Run(cfg, B, run_seed=3, queue_depth=3, auto_reset=True, num_slots=4, compact_features=True, mask_marginals=True)
        env = run.env
        acts, true_acts = (torch.zeros((B, 3), dtype=torch.int32, device=env.device) for _ in range(2))
        for t in range(4 * cfg.max_num_components):
            env.select_slot(t + 1)
            run.model.select(t + 1)
            a = _delayed_step(run, t, before, acts, true_acts, rng, p_bad=0.0)
            if t % 5 == 2:
                old = (env.obs_f64(), (env.reward, env.done, env.info_raw))  # views of the old set's selected slot
                _rebind_fresh(env)
                _settle(run, a, ("the step in flight at the rebind wrote the old tensors", t), obs=old)
                m = run.model  # a fresh set: nothing written, slot 0 selected
                m.R[:], m.D[:], m.I[:], m.fresh_rows[:], m.slot = 0.0, 0, np.nan, False, 0
                m.ld = ("slot", 0)
            else:
                _settle(run, a, ("rebind", t))
        run.close()


def _rebind_fresh(env):
    """pcbenv_bind_buffers_slots + pcbenv_bind_compact_features to a fresh set of tensors (what the constructor does)."""
    S, dev = env.num_slots, env.device
    env.traj = {k: torch.zeros_like(v) for k, v in env.traj.items()}
    env.traj_reward, env.traj_done = torch.zeros_like(env.traj_reward), torch.zeros_like(env.traj_done)
    env.traj_info = torch.full_like(env.traj_info, float("nan"))
    env.traj_marginals = {k: torch.zeros_like(v) for k, v in env.traj_marginals.items()}
    torch.cuda.current_stream(dev).synchronize()  # the fills are the caller's: done before the library hears of the tensors
    special = dict(reward=env.traj_reward, done=env.traj_done, info=env.traj_info, mask_orientation=env.traj_marginals.get("orientation"),
                   mask_rows=env.traj_marginals.get("rows"))
    bufs = _lib.PcbenvBuffers()
    for name in _lib.BUFFER_FIELDS:
        t = special[name] if name in special else env.traj.get(name)
        if env.compact_features and name in FEATURE_KEYS:
            t = None
        setattr(bufs, name, t.data_ptr() if t is not None else None)
    _lib.check(env._L.pcbenv_bind_buffers_slots(env._h, C.byref(bufs), S), env._h)
    if env.compact_features:
        cb = _lib.PcbenvCompactFeatures()
        for name in _lib.COMPACT_FIELDS:
            t = env.traj.get(name)
            setattr(cb, name, t.data_ptr() if t is not None else None)
        _lib.check(env._L.pcbenv_bind_compact_features(env._h, C.byref(cb)), env._h)
    env.slot = -1
    env.select_slot(0)
    env._last_done = env.done
