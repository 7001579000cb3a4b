"""The stream contract of the C ABI as a table, and the delay the GPU tests put in front of a call (plain module, no test).

CONTRACT has one row for every function of include/pcbenv.h with a `stream` parameter (tests/test_stream_cases.py
compares the keys with the header):

  "async"  the call enqueues on `stream` and returns; nothing of it may run on another stream, and it does not wait
  "sync"   the call is synchronous with `stream`: when it returns, everything enqueued on `stream` before it has run

lag(stream) enqueues a kernel that keeps `stream` busy for about LAG_MS milliseconds and touches no memory of ours: a
bounded delay (torch.cuda._sleep, a loop on the clock), not a wait for a flag.  A library call made right behind it
arrives while the stream is busy: if any part of it went to another stream, it would run early -- on inputs the tests
keep valid but wrong until the side stream has passed the lag -- and if the call waited for the stream, it would not
return before the lag is over.

LAG_MS follows from a measurement: at least 20 x the host time of the slowest "async" entry point on an idle stream and
at least 10 ms, so that a host thread that is held up for a moment does not turn "returned early" into a flake; at most
100 ms, so that a test module stays within seconds.  Timed with the library of the commit before this module, the
slowest call took 0.059 ms on the host (pcbenv_step with the on-device generator on, the worst of 25 calls in the slower of two runs;
profiles/stream_contract.txt has every figure): 20 x that is 1.2 ms, so the 10 ms floor decides, and 20 ms is twice the
floor -- 340 x the slowest call.  One delay of 20 ms was measured at 20 ms on the device.
"""
import contextlib

ASYNC = ("pcbenv_reset", "pcbenv_step", "pcbenv_sample_actions", "pcbenv_step_sampled", "pcbenv_rollout_sampled",
         "pcbenv_gather", "pcbenv_playout", "pcbenv_sample_logits", "pcbenv_evaluate_logits",
         "pcbenv_evaluate_logits_backward", "pcbenv_sample_axis", "pcbenv_evaluate_axis", "pcbenv_evaluate_axis_backward")
SYNC = ("pcbenv_load_instances", "pcbenv_get_state", "pcbenv_set_state", "pcbenv_get_instances", "pcbenv_queue_cursors",
        "pcbenv_instgen_device_enable", "pcbenv_instgen_device_status")
CONTRACT = {**{name: "async" for name in ASYNC}, **{name: "sync" for name in SYNC}}

LAG_MS = 20.0

_method = None  # ("sleep", cycles per ms) or ("links", elementwise kernels per ms, the scratch tensor)


def _timed(work):
    """Milliseconds `work()` keeps the current stream busy, by HIP events."""
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    work()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def _calibrate():
    """One timed call of torch.cuda._sleep (behind a first call that loads the kernel) gives its cycles per millisecond.
    Where that is no clock to rely on, a chain of elementwise kernels over one large scratch tensor of the module's own is
    timed instead, and a lag is as many links of it as the delay needs."""
    import torch
    if hasattr(torch.cuda, "_sleep"):
        probe = 2_000_000
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        ms = _timed(lambda: torch.cuda._sleep(probe))
        if 0.05 <= ms <= 500.0:  # 2e6 cycles of a clock between 4 MHz and 40 GHz
            return ("sleep", probe / ms)
    scratch = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")  # 256 MiB: beyond the caches
    scratch.add_(1.0)
    torch.cuda.synchronize()
    ms = _timed(lambda: [scratch.add_(1.0) for _ in range(8)])
    return ("links", 8.0 / max(ms, 1e-3), scratch)


def lag(stream, ms=LAG_MS):
    """Keeps `stream` busy for about `ms` milliseconds from where it is now.  Calibrated once per process."""
    import torch
    global _method
    with torch.cuda.stream(stream):
        if _method is None:
            _method = _calibrate()
        if _method[0] == "sleep":
            torch.cuda._sleep(int(ms * _method[1]))
        else:
            for _ in range(max(1, int(round(ms * _method[1])))):
                _method[2].add_(1.0)


def measured_lag_ms(stream, ms=LAG_MS):
    """What one lag(stream, ms) takes on the device, by HIP events (the figure profiles/stream_contract.txt records)."""
    import torch
    lag(stream, 0.01)  # calibration and kernel load are not part of it
    stream.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        t0.record()
        lag(stream, ms)
        t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


@contextlib.contextmanager
def lagged(stream, ms=LAG_MS):
    """Makes `stream` the current torch stream (the one BatchedPlacementEnv hands to the library) and yields the
    function the tests call before each library call: it puts one lag on `stream` and counts itself."""
    import torch

    def before():
        before.calls += 1
        lag(stream, ms)
    before.calls = 0
    with torch.cuda.stream(stream):
        yield before
