"""The live cases of the trainer tests (tests/trainer_cases.py: LIVE_CASES) meet, on the float64 statement alone and as
committed, the conditions under which a comparison with that statement sees every backward pass -- no GPU:

  * every ReLU (each tower layer, both head convolutions, the value dense layer) is on for a share of its pre-activations in
    [0.1, 0.9]; the one dense unit of D = 1 is on for at least one row and, among several rows, not for all;
  * |pre-tanh| within [0.05, 2] on every row (tanh' between 0.07 and 1, off the fixed point at 0), of both signs in a batch;
  * every trainable tensor's largest |data gradient| at least 1e-3; the policy tensors of the one row without a label exactly 0;
  * no pre-activation within 1e-4 of 0, so float32 and float64 take the same ReLU masks.

These are conditions on the inputs, not measurements: a case that misses one is replaced, the bound stays.  The two-step case
is held to them at both of its batches, the second at the weights the float64 optimiser leaves, per optimiser.  The live cases
of the scorer and of the epoch (tests/eval_cases.py: LIVE_CASES, EPOCH_LIVE_CASE) are held to the same conditions on their rows."""
import numpy as np
import pytest

from tests import eval_cases as EC
from tests.trainer_cases import (EPS, GAMES, LIVE_CASES, LIVE_LR, TWO_STEP_CASE, RefOptimizer, assert_live, live_case, make_batch,
                                 statement)


def test_the_cases_cover_the_shapes():
    assert {c[1] for c in LIVE_CASES} == {0, 1, 2, 9} and {c[2] for c in LIVE_CASES} == {1, 16, 64}
    assert {c[3] for c in LIVE_CASES} == {1, 2, 6, 130} and {c[0] for c in LIVE_CASES} == set(GAMES)
    assert {c[6] for c in LIVE_CASES if c[3] == 1} == {True, False} and len(set(LIVE_CASES)) == len(LIVE_CASES)


@pytest.mark.parametrize("case", LIVE_CASES, ids=str)
def test_case_is_live(case):
    _game, _R, D, B, _ws, _bs, terminal_last = case
    ref = live_case(case)
    assert all(v.dtype == np.float32 for v in ref["w"].values())
    assert_live(ref["want"], B, D, B == 1 and terminal_last, case)
    print(case, "float32 statement %.3g tolerance %.3g" % (ref["figure"], ref["tol"]))
    assert 0 < ref["figure"] and ref["tol"] <= 1e-5


@pytest.mark.parametrize("kind", ["adam", "momentum", "sgd"])
def test_second_step_of_the_two_step_case_is_live(kind):
    game, _R, D, B, _ws, b_seed, terminal_last = TWO_STEP_CASE
    _g, H, Wd, A = GAMES[game]
    ref = live_case(TWO_STEP_CASE)
    w64 = {k: np.asarray(v, dtype=np.float64) for k, v in ref["w"].items()}
    after = RefOptimizer(kind, 0.9).apply(w64, ref["want"][2], LIVE_LR)
    second = make_batch(H, Wd, A, B, b_seed + 1, terminal_last=terminal_last)
    assert_live(statement({k: v.astype(np.float32) for k, v in after.items()}, *second, EPS, parts=True), B, D, False, (kind, "step 1"))


# ---- the scorer's and the epoch's live cases --------------------------------------------------------------------------------------
def test_the_scorer_cases_cover_the_shapes():
    assert {c[1] for c in EC.LIVE_CASES} == {0, 2, 9} and {c[2] for c in EC.LIVE_CASES} == {1, 64}
    assert {c[3] for c in EC.LIVE_CASES} == {1, 2, 130} and {c[0] for c in EC.LIVE_CASES} == set(GAMES)


@pytest.mark.parametrize("case", EC.LIVE_CASES, ids=str)
def test_scorer_case_is_live(case):
    """The same conditions on the scorer's rows, through the training statement of those rows (no noise): a scorer has no backward
    pass, but rows on which training would be live are rows whose value, se and ce move with every weight."""
    _name, _R, D, n, _ws = case
    ref = EC.live_case(case)
    boards, z, pi = ref["rows"]
    assert_live(statement(ref["w"], boards, z, pi, None, 0.0, parts=True), n, D, n == 1 and not pi.any(), case)
    value = ref["want"]["rows"][:, 0]
    print(case, "values", value.min(), value.max(), "float32 statement", ref["figure"], "tolerance", ref["tol"])
    assert (np.abs(value) < 0.95).any() and all(0 < f for f in ref["figure"]) and all(t <= 1e-5 for t in ref["tol"])
    if n >= 2:      # what tests/test_gpu_trainer_eval.py says of its rows: a row without a label is among them
        assert not ref["want"]["has"].all() and ref["want"]["has"].any()


def test_epoch_case_is_live():
    _name, _R, D, batch, _ws, _first = EC.EPOCH_LIVE_CASE
    ref = EC.epoch_live_case()
    assert_live(ref["want"], batch, D, False, EC.EPOCH_LIVE_CASE)
    print("float32 statement %.3g tolerance %.3g" % (ref["figure"], ref["tol"]))
    assert 0 < ref["figure"] and ref["tol"] <= 1e-5
