"""The UNet launch schedules (said_amd/csrc/unet_sched.cpp) against the recorded ones (tests/golden/unet_sched.json).

The file was recorded before the schedules' shared steps were folded into one builder each: for every case — precision mode, shape, debug options —
the launches of one UNet evaluation in order (kernel family, epilogue, tile shape, algorithmic bytes and flops) and the nodes of the guided step graph.
A host-side change that is meant to keep the schedules must keep all of it; a change that is meant to alter a schedule records the file again
(tests/golden/make_golden_sched.py) and says so.
"""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_golden_sched", os.path.join(GOLDEN, "make_golden_sched.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

with open(rec.FIXTURE) as _f:
    _doc = json.load(_f)
assert tuple(_doc["stage_fields"]) == rec.FIELDS
RECORDED = {c["name"]: c for c in _doc["cases"]}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    return rec.make_model(dev)


def test_the_recorded_cases_are_the_script_s():
    assert [(c[0], c[1], c[2], c[3], c[4], c[5]) for c in rec.CASES] == \
           [(c["name"], c["precision"], c["Be"], c["T"], c["cfg_clips"], c["options"]) for c in RECORDED.values()]
    hit = {h for c in RECORDED.values() for h in c["functions"]}
    assert hit >= {"run_transformer", "run_transformer_tm", "run_transformer_hybrid", "battn", "chain", "resblock_range_split", "proj_out_range_split"}


@pytest.mark.parametrize("case", rec.CASES, ids=[c[0] for c in rec.CASES])
def test_launch_schedule_is_the_recorded_one(model, dev, case):
    want = RECORDED[case[0]]
    got = rec.record_case(model, dev, case)   # (options and precision are restored by its context manager, also when it raises)
    print(f"{case[0]}: {len(got['stages'])} launches ({len(want['stages'])} recorded), {got['graph_nodes']} graph nodes ({want['graph_nodes']} recorded)")
    assert got["graph_nodes"] == want["graph_nodes"]
    assert [s[:4] for s in got["stages"]] == [s[:4] for s in want["stages"]]   # kind, epi, NB, KS of every launch, in order
    for i, (a, b) in enumerate(zip(got["stages"], want["stages"])):
        for k in (4, 5):   # bytes, flops: host doubles of unchanged expressions, the margin is for reassociation alone
            assert abs(a[k] - b[k]) <= 1e-9 * abs(b[k]), f"launch {i} {rec.FIELDS[k]}: {a[k]!r} != {b[k]!r}"
