"""Seeded random call sequences over the whole call alphabet of a handle, against the host model of
tests/handle_model.py: after every call every observation tensor, reward, done, info, the mask marginals and
`mask_bits()` must equal the CPU oracle's, bit for bit.  The hand-written tests pin one call order per feature; this
module explores "what was called before" x "what is called now" (tests/test_handle_model.py checks, without a GPU, that
the schedules reach every op and every ordered pair of ops).  A failure names the setup, the seed and the ops executed
so far; `handle_model.run_sequence(setup, seed)` reproduces it."""
import pytest

from handle_model import SETUPS, run_sequence

pytestmark = pytest.mark.gpu

OP_COUNTS = {}  # setup -> ops executed by kind (printed per setup; profiles/call_sequences.txt records them)


@pytest.mark.parametrize("name,seed", [(name, seed) for name, s in SETUPS.items() for seed in s.seeds])
def test_call_sequence(name, seed):
    from collections import Counter
    counts = OP_COUNTS.setdefault(name, Counter())
    try:
        run_sequence(SETUPS[name], seed, counts)
    finally:
        if seed == SETUPS[name].seeds[-1]:
            print(f"SEQ-OPS {name} B={SETUPS[name].B} seeds={len(SETUPS[name].seeds)} total={sum(counts.values())} "
                  + " ".join(f"{k}={v}" for k, v in sorted(counts.items())))
