"""No GPU: the host side of bb_examples_score -- the float64 statement of a scored row (tests/score_cases.py) against the statement
of the trainer's scorer (tests/eval_cases.py) on Connect4 rows, the hand-built corners under chosen logits, the refusals that
need no device, and the front end's argument check.

Where the two statements can agree.  Both are given the same float32 logits and values and the same float32 labels, so the
counts and every bit are equal and the cross entropies agree to float64 rounding (1e-12).  The squared error cannot: the entry
point defines se as the float32 figure (one subtraction, one multiplication: what the kernel writes, bit for bit), eval_cases
takes it in float64.  Each float32 se is within 3 * 2^-24 of the float64 one (two roundings, the first one doubled by the
square), so that is the bound on the sums; a wrong operation order or a missing rounding shows in the GPU file, bit for bit.

An engine cannot exist without a GPU (bb_create refuses), so of the BB_ERR_ARG answers only the null-engine ones are reached
here; the others, and bb_examples_score_workspace's growth, are in tests/test_gpu_examples_score.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from blackbird_amd import Blackbird, _lib
from blackbird_amd.training import DeviceExamples, MergedExamples
from tests import eval_cases as EC
from tests import score_cases as SC

C4, TTT, DC = SC.C4, SC.TTT, SC.DC


def _net_outputs(game, n, seed):
    rng = np.random.RandomState(seed)
    A = _lib.game_info(game).A
    return (rng.randn(n, A) * 2.0).astype(np.float32), np.tanh(rng.randn(n)).astype(np.float32)


def test_statement_against_the_trainer_scorers_statement(monkeypatch):
    rec = EC.records(C4)
    logits, values = _net_outputs(C4, len(rec), 3)
    values[7] = 0.0                                                   # value == 0 disagrees with either sign
    mine = SC.statement(C4, logits, values, rec)
    monkeypatch.setattr(EC, "forward", lambda w0, boards, dtype=np.float64: (values.astype(dtype), logits.astype(dtype)))
    pi = np.stack([SC.label(C4, r) for r in rec])
    theirs = EC.statement(None, None, rec["z"], pi)
    has, top1, decided, sign_ok, counted = EC.bits(mine["flags"])
    assert counted.all() and mine["ok"].all() and (rec["total"] == 0).any()
    for got, k in ((has, "has"), (top1, "top1"), (decided, "decided"), (sign_ok, "sign_ok")):
        assert np.array_equal(got, theirs[k]), k
    for k in EC.COUNTS:
        assert mine["totals"][k] == theirs["totals"][k], k
    assert np.array_equal(mine["rows"][:, 0], theirs["rows"][:, 0])
    err = np.abs(mine["rows"][:, 2] - theirs["rows"][:, 2]).max()
    print("ce: largest difference %.3g" % err)
    assert err <= 1e-12 * max(1.0, np.abs(theirs["rows"][:, 2]).max())
    assert abs(mine["totals"]["ce_sum"] - theirs["totals"]["ce_sum"]) <= 1e-12 * max(1.0, abs(theirs["totals"]["ce_sum"]))
    se_err = abs(mine["totals"]["se_sum"] - theirs["totals"]["se_sum"])
    print("se_sum: float32 figures %.17g float64 %.17g" % (mine["totals"]["se_sum"], theirs["totals"]["se_sum"]))
    assert se_err <= 3 * 2.0 ** -24 * theirs["totals"]["se_sum"]
    d = values - rec["z"].astype(np.float32)                          # the float32 figure, exactly
    assert np.array_equal(mine["rows"][:, 1], (d * d).astype(np.float64)) and d.dtype == np.float32


@pytest.mark.parametrize("game", [C4, TTT, DC])
def test_hand_built_rows_under_chosen_logits(game):
    rec, at = SC.corners(game)
    A = _lib.game_info(game).A
    index = np.array([at["tie"], -1, at["terminal"], len(rec), at["too_many"], at["tie"]] + ([at["bad_action"]] if game == DC else []))
    n = len(index)
    flat = np.zeros((n, A), dtype=np.float32)
    values = np.full(n, 0.5, dtype=np.float32)
    want = SC.statement(game, flat, values, rec, index)
    assert want["ok"].tolist() == [True, False, True, False, False, True] + ([False] if game == DC else [])
    assert not want["rows"][~want["ok"]].any() and not want["flags"][~want["ok"]].any()
    assert want["totals"]["rows"] == 3 and want["totals"]["policy_rows"] == 2
    # constant logits: ce = log A (the label sums to 1 up to its float32 roundings); the logits' first maximum is action 0
    assert abs(want["rows"][0, 2] - np.log(A)) <= 1e-6 * np.log(A) and want["rows"][2, 2] == 0.0
    assert not want["flags"][2] & _lib.ROW_HAS_POLICY and want["flags"][2] & _lib.ROW_COUNTED
    assert not want["flags"][0] & _lib.ROW_TOP1
    # the tie: the label's first maximum in action order, wherever it stands in the record's list
    first, later = (100, 500) if game == DC else (2, 5)
    assert int(np.argmax(SC.label(game, rec[at["tie"]]))) == first
    assert SC.label(game, rec[at["tie"]])[first] == SC.label(game, rec[at["tie"]])[later]
    for peak, hit in ((first, True), (later, False)):
        lg = flat.copy()
        lg[:, peak] = 1.0
        flags = SC.statement(game, lg, values, rec, index)["flags"]
        assert bool(flags[0] & _lib.ROW_TOP1) is hit and bool(flags[5] & _lib.ROW_TOP1) is hit and not flags[2] & _lib.ROW_TOP1
    # z = 1 on the tie row, value 0.5: decided, sign right; se = 0.25 exactly
    assert want["flags"][0] & _lib.ROW_DECIDED and want["flags"][0] & _lib.ROW_SIGN_OK and want["rows"][0, 1] == 0.25
    assert {int(z) for z in rec["z"][[at[k] for k in at if k not in ("too_many", "bad_action")]]} == {-1, 0, 1}


def test_refusals_that_need_no_device():
    L = _lib.lib()
    out = C.c_uint64(7)
    assert L.bb_examples_score_workspace(None, 4, C.byref(out)) == _lib.ERR_ARG and out.value == 7
    assert L.bb_examples_score(None, 0, None, 0, None, None, None, None, None, None, 0, None) == _lib.ERR_ARG
    assert "engine" in _lib.last_error()
    assert L.bb_examples_score(None, 4, None, -1, None, None, None, None, None, None, 0, None) == _lib.ERR_ARG


def test_entry_points_are_bound():
    for name in ("bb_examples_score", "bb_examples_score_workspace"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert callable(_lib.Engine.score_examples) and callable(_lib.Engine.score_workspace) and callable(DeviceExamples.score_with)


def test_front_end_checks_its_scorer_before_it_touches_the_model():
    with pytest.raises(ValueError, match="scorer"):
        Blackbird.EvaluateDeviceExamples(None, examples=None, scorer="bogus")


def test_what_is_not_a_records_source_or_an_engine():
    rec = EC.records(C4)[:12]
    ex = DeviceExamples.from_records(C4, rec, "cpu")
    merged = ex.merged()
    assert type(merged) is MergedExamples
    with pytest.raises(ValueError, match="records source"):
        merged.score_with(None)
    with pytest.raises(ValueError, match="Engine"):
        ex.score_with(object())
    assert torch.equal(ex.records, DeviceExamples.from_records(C4, rec, "cpu").records)
