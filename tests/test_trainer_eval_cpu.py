"""No GPU: the host side of the held-out evaluation -- DeviceExamples.split_games on CPU records of all three games, the float32
torch statement of the per-row figures (Trainer.evaluate_tensors) against the float64 one (tests/eval_cases.py) under the `close`
rule of tests/trainer_cases.py (1e-5 relative to max(1, largest |entry|)), and the new entry points in the binding list."""
import numpy as np
import pytest
import torch

from blackbird_amd import _lib
from blackbird_amd import weights as W
from blackbird_amd.training import DeviceExamples, Trainer, eval_summary
from tests import eval_cases as EC
from tests.merge_cases import C4, DC, TTT
from tests.trainer_cases import GAMES, close, make_batch


# ---- split_games -----------------------------------------------------------------------------------------------------------------
def _ids(ex):
    return ex.records[:, :4].contiguous().view(torch.int32).reshape(-1).numpy()


@pytest.mark.parametrize("game", [C4, TTT, DC])
@pytest.mark.parametrize("n_games,fraction,want", [(10, 0.1, 1), (10, 0.3, 3), (7, 0.5, 4), (10, 0.0, 1), (10, 1.0, 9), (2, 0.5, 1)])
def test_split_games(game, n_games, fraction, want):
    rec = EC.any_game_records(game, n_games, 3, 5)
    rec = rec[np.random.RandomState(1).permutation(len(rec))]            # games interleaved: order must still be kept
    ex = DeviceExamples.from_records(game, rec, "cpu")
    before = np.random.get_state()
    train, held = ex.split_games(fraction, 4)
    after = np.random.get_state()
    assert np.array_equal(before[1], after[1]) and before[2:] == after[2:]     # numpy's global generator is not touched
    assert type(train) is DeviceExamples and train.game == held.game == game
    ids, tid, hid = _ids(ex), _ids(train), _ids(held)
    assert want == min(max(int(round(fraction * n_games)), 1), n_games - 1)
    assert len(np.unique(hid)) == want and len(np.unique(tid)) == n_games - want
    assert not set(tid) & set(hid) and len(train) + len(held) == len(ex)        # disjoint, every game whole on one side
    uniq = np.unique(ids)
    assert sorted(np.unique(hid)) == sorted(np.random.RandomState(4).permutation(uniq)[:want])
    is_held = np.isin(ids, np.unique(hid))
    assert np.array_equal(held.records.numpy(), ex.records.numpy()[is_held])    # order kept, bytes kept
    assert np.array_equal(train.records.numpy(), ex.records.numpy()[~is_held])
    again = ex.split_games(fraction, 4)
    assert torch.equal(again[0].records, train.records) and torch.equal(again[1].records, held.records)


def test_split_games_seed_and_errors():
    rec = EC.any_game_records(C4, 12, 2, 6)
    ex = DeviceExamples.from_records(C4, rec, "cpu")
    helds = {tuple(np.unique(_ids(ex.split_games(0.25, seed)[1]))) for seed in range(6)}
    assert len(helds) > 1                                                        # another seed, another choice
    one = DeviceExamples.from_records(C4, EC.any_game_records(C4, 1, 5, 7), "cpu")
    with pytest.raises(ValueError, match="two games"):
        one.split_games(0.5, 0)
    with pytest.raises(ValueError, match="two games"):
        DeviceExamples(C4, torch.zeros((0, rec.dtype.itemsize), dtype=torch.uint8)).split_games(0.5, 0)


# ---- Trainer.evaluate_tensors against the float64 statement ---------------------------------------------------------------------
@pytest.mark.parametrize("name,R,D,B", [("connect4", 0, 16, 5), ("connect4", 2, 7, 9), ("tictactoe", 2, 16, 6), ("tictactoe", 9, 64, 3)])
def test_torch_evaluation_against_the_statement(name, R, D, B):
    _game, H, Wd, A = GAMES[name]
    w0 = W.init_weights(3, 16, R, D, A, seed=5, perturb=True)
    boards, ev, pl, _noise = make_batch(H, Wd, A, B, 31)                          # the last row: a terminal example, pi = 0
    pl[0, :] = 0.0
    pl[0, [2, 4]] = 0.5                                                           # tied top shares: the first maximum counts
    want = EC.statement(w0, boards, ev, pl)
    tr = Trainer(w0, device="cpu")
    t = lambda x: torch.tensor(np.asarray(x, dtype=np.float32))  # noqa: E731
    got = tr.evaluate_tensors(t(boards), t(ev), t(pl), rows=True)
    close(got["per_row"].numpy(), want["rows"], (name, "rows"))
    assert want["rows"][-1, 2] == 0.0 and got["per_row"][-1, 2] == 0.0 and not want["has"][-1]
    has, top1, decided, sign_ok, counted = EC.bits(got["flags"].numpy())
    assert counted.all() and np.array_equal(has, want["has"]) and np.array_equal(decided, want["decided"])
    room = want["has"] & want["top1_room"]
    assert np.array_equal(top1[room], want["top1"][room]) and not top1[~want["has"]].any()
    room = want["decided"] & want["sign_room"]
    assert np.array_equal(sign_ok[room], want["sign_ok"][room]) and not sign_ok[~want["decided"]].any()
    for k in ("rows", "policy_rows", "decided"):
        assert got[k] == want["totals"][k], k
    assert got["top1"] == int(top1.sum()) and got["sign_ok"] == int(sign_ok.sum())
    close(got["se_sum"], want["totals"]["se_sum"], (name, "se_sum"))
    close(got["ce_sum"], want["totals"]["ce_sum"], (name, "ce_sum"))
    close(got["value_mse"], want["totals"]["se_sum"] / B, (name, "value_mse"))
    close(got["policy_ce"], want["totals"]["ce_sum"] / want["totals"]["policy_rows"], (name, "policy_ce"))
    assert got["top1_rate"] == got["top1"] / got["policy_rows"] and got["sign_rate"] == got["sign_ok"] / got["decided"]
    # evaluation moves nothing
    for k, v in tr.export().items():
        assert np.array_equal(v, w0[k]), k


def test_means_over_zero_rows_are_nan():
    out = eval_summary(0, 0, 0, 0, 0, 0.0, 0.0)
    assert all(np.isnan(out[k]) for k in ("value_mse", "policy_ce", "top1_rate", "sign_rate")) and out["rows"] == 0
    w0 = W.init_weights(3, 16, 0, 16, 7, seed=5, perturb=True)
    got = Trainer(w0, device="cpu").evaluate_tensors(torch.zeros((0, 6, 7, 3)), torch.zeros(0), torch.zeros((0, 7)))
    assert got["rows"] == 0 and np.isnan(got["value_mse"])


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_bound():
    for name in ("bb_trainer_eval", "bb_trainer_eval_tensors"):
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert np.dtype(_lib.EVAL_TOTALS_DTYPE).itemsize == 56
    assert callable(_lib.trainer_eval) and callable(_lib.trainer_eval_tensors)
