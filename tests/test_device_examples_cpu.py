"""CPU-side checks of training from device-resident examples (blackbird_amd/training.py: epoch_order, DeviceExamples;
bb_examples_to_batch): the epoch's order is TrainWithExamples' own draw, an empty batch needs no GPU, and the new entry
point is declared, exported and bound (tests/test_abi.py::test_header_symbols_exported compares the three lists)."""
import numpy as np
import pytest
import torch

from blackbird_amd import _lib
from blackbird_amd.training import DeviceExamples, epoch_order


@pytest.mark.parametrize("n,B", [(10, 4), (8, 8), (3, 4), (1, 1)])  # (3, 4): no whole batch, an empty order
@pytest.mark.parametrize("seed", [0, 7])
def test_epoch_order_is_the_draw_of_train_with_examples(n, B, seed):
    np.random.seed(seed)
    got = epoch_order(n, B)
    state_got = np.random.get_state()
    np.random.seed(seed)
    want = np.random.choice(n, n - n % B, replace=False)  # Blackbird.TrainWithExamples
    state_want = np.random.get_state()
    assert got.dtype == want.dtype and np.array_equal(got, want) and len(got) == n - n % B
    assert state_got[0] == state_want[0] and np.array_equal(state_got[1], state_want[1]) and state_got[2:] == state_want[2:]


def test_empty_batch_needs_no_gpu():
    for game in (_lib.GAME_CONNECT4, _lib.GAME_TICTACTOE, _lib.GAME_DRAGONCHESS):
        _lib.examples_to_batch(game, 0, None, 0)
        _lib.examples_to_batch(game, 5, None, 0, index=None, boards=None, policy=None, value=None, bad=None, stream=0)
    with pytest.raises(ValueError):
        _lib.examples_to_batch(_lib.GAME_CONNECT4, 5, None, -1)
    with pytest.raises(ValueError):
        _lib.examples_to_batch(_lib.GAME_CONNECT4, 5, None, 3)  # no records (checked before anything is launched)
    assert "bb_examples_to_batch" in _lib.EXPORTS


def test_device_examples_bookkeeping_on_the_host():
    """Everything of DeviceExamples that is not the kernel: shapes, cat, the index range check, the empty batch."""
    game = _lib.GAME_CONNECT4
    gi = _lib.game_info(game)
    rec = np.zeros(5, dtype=_lib.example_dtype(game))
    rec["ply"] = np.arange(5)
    a = DeviceExamples.from_records(game, rec[:2], "cpu")
    b = DeviceExamples.from_records(game, rec[2:], "cpu")
    both = DeviceExamples.cat([a, b])
    assert (len(a), len(b), len(both)) == (2, 3, 5) and both.bad() == 0
    assert both.records.numpy().tobytes() == rec.tobytes()
    boards, value, policy = both.batch(np.zeros(0, dtype=np.int64))
    assert boards.shape == (0, gi.H, gi.W, gi.C) and value.shape == (0,) and policy.shape == (0, gi.A)
    assert boards.dtype == value.dtype == policy.dtype == torch.float32
    for wrong in ([5], [-1], torch.tensor([0, 5])):
        with pytest.raises(IndexError):
            both.batch(wrong)
    with pytest.raises(_lib.BlackbirdHipError):  # records on the host: there is no CPU path, and none is faked
        both.batch([0, 1])
    with pytest.raises(ValueError):
        DeviceExamples(game, torch.zeros((3, gi.example_bytes + 16), dtype=torch.uint8))
    with pytest.raises(ValueError):
        DeviceExamples.cat([a, DeviceExamples.from_records(_lib.GAME_TICTACTOE,
                                                           np.zeros(1, dtype=_lib.example_dtype(_lib.GAME_TICTACTOE)), "cpu")])
