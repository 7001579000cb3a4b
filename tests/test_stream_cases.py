"""The stream contract table (tests/stream_cases.py) against the header, and the GPU tests of tests/test_streams_gpu.py
against the table.  Needs no GPU."""
import ast
import os
import re

import stream_cases as sc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _functions_with_a_stream_parameter():
    """As tests/test_abi.py reads the header: comments stripped, then every declaration `pcbenv_name(...)` up to its `;`."""
    text = open(os.path.join(REPO, "include", "pcbenv.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = re.findall(r"\b(pcbenv_[a-z_]+)\s*\(([^;{]*)\)\s*;", text)
    assert len(decls) >= 30, "the header no longer parses the way this test reads it"
    return sorted(name for name, params in decls if re.search(r"\bvoid\s*\*\s*stream\b", params))


def test_the_table_has_one_row_per_function_with_a_stream_parameter():
    names = _functions_with_a_stream_parameter()
    assert len(names) == len(set(names)) == 20
    assert sorted(sc.CONTRACT) == names, (sorted(set(names) - set(sc.CONTRACT)), sorted(set(sc.CONTRACT) - set(names)))
    assert set(sc.CONTRACT.values()) == {"async", "sync"}
    assert not set(sc.ASYNC) & set(sc.SYNC) and len(sc.CONTRACT) == len(sc.ASYNC) + len(sc.SYNC)


def test_the_header_states_the_class_of_every_row():
    """The "Streams" paragraph of the header names every row, the enqueue-only ones before the synchronous ones."""
    text = open(os.path.join(REPO, "include", "pcbenv.h")).read()
    para = text[text.index(" * Streams."):text.index("What each entry point replaces")]
    para = re.sub(r"\s*\n \*\s*", " ", para)
    para = para.replace("pcbenv_evaluate_logits[_backward]", "pcbenv_evaluate_logits, pcbenv_evaluate_logits_backward")
    para = para.replace("pcbenv_evaluate_axis[_backward]", "pcbenv_evaluate_axis, pcbenv_evaluate_axis_backward")
    enqueue = para[para.index("These only enqueue"):para.index("These move data")]
    synchronous = para[para.index("These move data"):para.index("pcbenv_set_option")]
    named = lambda part: set(re.findall(r"pcbenv_[a-z_]+", part))
    assert named(enqueue) == set(sc.ASYNC)
    assert named(synchronous) == set(sc.SYNC)


def test_the_lag_is_within_the_bounds_the_contract_tests_need():
    assert 10.0 <= sc.LAG_MS <= 100.0


def test_every_row_is_driven_by_a_gpu_test():
    import test_streams_gpu as gpu
    tree = ast.parse(open(gpu.__file__).read())
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    assert set(gpu.DRIVES) == tests, "DRIVES and the test functions of tests/test_streams_gpu.py name different tests"
    assert gpu.pytestmark.name == "gpu"
    driven = {}
    for test, rows in gpu.DRIVES.items():
        for case, names in (rows.items() if isinstance(rows, dict) else [(None, rows)]):
            assert names and set(names) <= set(sc.CONTRACT), (test, case, sorted(set(names) - set(sc.CONTRACT)))
            for n in names:
                driven.setdefault(n, []).append(test if case is None else f"{test}[{case}]")
    missing = sorted(set(sc.CONTRACT) - set(driven))
    assert not missing, f"no GPU test drives {missing}"
    # the parametrised tests declare exactly the ids they run
    assert set(gpu.DRIVES["test_every_async_call_runs_on_the_stream_it_was_given"]) == set(gpu.ENV_CASES) | set(gpu.POLICY_CASES)
    for n in sc.ASYNC:  # the placement test and the early-return test both cover every async row
        assert any(t.startswith("test_every_async_call_runs_on_the_stream_it_was_given[") for t in driven[n]), n
        assert "test_async_calls_return_before_the_stream_reaches_them" in driven[n], n
    for n in sc.SYNC:
        assert "test_async_calls_return_before_the_stream_reaches_them" in driven[n], n


def test_the_generator_protocol_restatement():
    """gen_protocol_counts on sequences worked out by hand from csrc/pcb_gen.hip (queue_depth 3)."""
    from test_streams_gpu import gen_protocol_counts
    # one record per launch: a fill starts once half the queue is used (after launch 2), is waited for before launch 4
    assert gen_protocol_counts([1], 3) == (0, 0)
    assert gen_protocol_counts([1, 1], 3) == (1, 0)
    assert gen_protocol_counts([1, 1, 1, 1], 3) == (2, 1)
    # three at once: every launch needs a fill of its own snapshot
    assert gen_protocol_counts([3, 3], 3) == (2, 1)
