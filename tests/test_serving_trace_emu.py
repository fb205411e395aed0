"""The serving engine's requests, launch for launch: tests/golden/serving_trace.json holds what every kind of request handed to the
backend BEFORE the serving host code was last changed -- per request the graph key, the noise shapes and commit count, the op
names and a digest of each call's arguments (tests/golden/make_serving_trace.py, which documents the request list).  The same
requests are recorded again here, once per session, through the emulation backend on the CPU and compared: a refactor of the host
code must leave every entry as it is.  The comparison itself is shown to report a dropped call, two swapped calls and a changed slot
list with their request and call index."""
import copy
import importlib.util
import json
import os

import pytest


@pytest.fixture(scope="module")
def M(golden_dir):
    spec = importlib.util.spec_from_file_location("make_serving_trace", os.path.join(golden_dir, "make_serving_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "serving_trace.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def trace(M):
    """The requests on the tree under test, with the full signatures (read-only)."""
    return M.record()


def test_request_list(M, recorded):
    """The file holds the requests of the recorder, all of them, and a count of 9 takes the chunk loop's second round."""
    from mmdyn_hip import ops
    names = [r[0] for r in M.engine_requests()] + [r[0] for r in M.problem_requests()[1]]
    assert list(recorded) == names
    assert M.COUNTS[0] <= ops.ROW_GROUPS_MAX < M.COUNTS[1]
    for r in ("score/samples={}", "rollout/samples={}"):
        few, many = (recorded[r.format(n)]["ops"].split().count("bce_logits_rows_groups") for n in M.COUNTS)
        assert many == 2 * few > 0, r
    assert recorded["plan/per_row"]["ops"].split().count("mse_rows_groups") == 2


def test_trace_is_unchanged(M, recorded, trace):
    assert M.compare(recorded, M.digested(trace)) == []


def test_problem_layer(M, recorded, trace):
    """The four serving methods of the problem layer: the model's mode around the call (``complete`` leaves it alone, the others
    restore it) and one engine per attribute across calls -- as recorded, and as the methods document."""
    for name in (r for r in trace if r.startswith("problem/")):
        assert trace[name]["training"] == recorded[name]["training"] == [True, True, True], name
        assert trace[name]["same_engine"] is True is recorded[name]["same_engine"], name


def test_comparison_sees_a_difference(M, recorded, trace):
    """A trace with one call dropped, one with two calls swapped and one with a slot list changed: each is reported with its
    request and call index, and nothing else is."""
    r = "score/samples=9"
    calls = trace[r]["calls"]
    i = next(k for k, (op, _) in enumerate(calls) if op == "bce_logits_rows_groups")
    assert calls[i][1][0][3] == list(range(8))                                      # (the slot list of the first eight draws)
    mutate = lambda edit: M.digested(dict(trace, **{r: dict(trace[r], calls=edit(copy.deepcopy(calls)))}))

    d = next(k for k, (op, _) in enumerate(calls) if op == "mse_rows_groups")      # (the call after it is another op)
    dropped = mutate(lambda c: c[:d] + c[d + 1:])
    assert M.compare(recorded, dropped) == [f"request {r}, call {d}, op mse_rows_groups: {calls[d + 1][0]} in its place "
                                            f"({len(calls) - 1} calls, recorded {len(calls)})"]
    j = next(k for k in range(len(calls) - 1) if calls[k][0] != calls[k + 1][0])
    swapped = mutate(lambda c: c[:j] + [c[j + 1], c[j]] + c[j + 2:])
    assert M.compare(recorded, swapped) == [f"request {r}, call {j}, op {calls[j][0]}: {calls[j + 1][0]} in its place "
                                            f"({len(calls)} calls, recorded {len(calls)})"]

    def other_slots(c):
        c[i][1][0][3] = [0]
        return c
    assert M.compare(recorded, mutate(other_slots)) == [f"request {r}, call {i}, op bce_logits_rows_groups: its arguments differ "
                                                        f"({len(calls)} calls, recorded {len(calls)})"]
    # ... and a key, a draw or a commit count that differs is reported with its request
    other = copy.deepcopy(recorded)
    other[r]["key"], other[r]["noise"], other[r]["commits"] = "()", [[9, 3, 64], [1]], 2
    assert [d.split(":")[0] for d in M.compare(recorded, other)] == [f"request {r}"] * 3
