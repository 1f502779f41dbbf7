"""CPU-side checks of merging duplicate positions in example records (training.merge_records_host, MergedExamples on host
records, bb_examples_merge*'s argument checks): the numpy statement against a naive dict loop, the hand cases of the definition,
its properties, and everything that has to be refused before a device call."""
import numpy as np
import pytest
import torch

from blackbird_amd import _lib
from blackbird_amd.training import DeviceExamples, MergedExamples, merge_records_host
from tests import merge_cases as MC
from tests.merge_cases import C4, DC, TTT

GAMES = [C4, TTT]


def _empty(game):
    H, W = MC.SHAPE[game][:2]
    return np.zeros((H, W), dtype=np.int8)


@pytest.mark.parametrize("game", GAMES)
def test_numpy_statement_is_the_dict_loop(game):
    rec = MC.dict_loop_input(game)
    got, want = merge_records_host(game, rec), MC.dict_merge(game, rec)
    MC.same_merge(got, want)
    for g, dt in zip(got, (np.int32, np.int32, np.int32, np.int32, np.uint64, np.uint64)):
        assert g.dtype == dt
    count = want[2]
    assert len(count) < len(rec) and count.max() > 2 and (count == 1).any()  # duplicates and singles are both there
    assert (rec["total"] == 0).any()


@pytest.mark.parametrize("game", GAMES)
def test_hand_cases(game):
    A, S = MC.SHAPE[game][3:]
    e = _empty(game)
    b = MC.play(game, e, 0, 1)            # one stone of player 1
    c = MC.play(game, b, 1, 2)
    v = lambda *x: np.array(list(x) + [0] * (A - len(x)), dtype=np.uint32)  # noqa: E731
    rows = [
        MC.record(game, b, 2, prev=1, z=1, visits=v(3, 4), game_id=5, ply=1),     # 0
        MC.record(game, b, 1, prev=1, z=-1, visits=v(1, 1)),                     # 1: same cells, the other side to move
        MC.record(game, b, 2, prev=0, z=-1, visits=v(10, 0, 6), game_id=9, ply=7),  # 2: record 0's key; other prev, game, ply
        MC.record(game, c, 1, prev=2, z=1),                                      # 3: a terminal record (total 0)
        MC.record(game, b, 2, prev=1, z=1, visits=v(100, 100), n_children=S + 1),  # 4: malformed, although its key is record 0's
        MC.record(game, c, 1, prev=2, z=-1),                                     # 5: the terminal position again
        MC.record(game, b, 2, prev=2, z=1, visits=v(0, 1)),                      # 6: record 0's key once more
    ]
    rec = MC.stack(rows, game)
    group, rep, count, zsum, total, visits = merge_records_host(game, rec)
    assert group.tolist() == [0, 1, 0, 2, -1, 2, 0]
    assert rep.tolist() == [0, 1, 3] and count.tolist() == [3, 1, 2] and zsum.tolist() == [1, -1, 0]
    assert total.tolist() == [7 + 16 + 1, 2, 0]
    assert visits[0].tolist() == v(13, 5, 6).tolist() and visits[1].tolist() == v(1, 1).tolist() and not visits[2].any()
    value, policy = MC.rows_of(rec, (group, rep, count, zsum, total, visits))
    assert value.tolist() == [np.float32(1 / 3), -1.0, 0.0] and not policy[2].any()
    assert np.array_equal(policy[0], (v(13, 5, 6).astype(np.float64) / 24.0).astype(np.float32))
    assert np.array_equal(policy[1], (v(1, 1) / 2).astype(np.float32))
    MC.same_merge((group, rep, count, zsum, total, visits), MC.dict_merge(game, rec))


def _by_key(rec, merged):
    group, rep, count, zsum, total, visits = merged
    return {MC.key_of(rec[rep[g]]): (int(count[g]), int(zsum[g]), int(total[g]), tuple(int(x) for x in visits[g]))
            for g in range(len(rep))}


@pytest.mark.parametrize("game", GAMES)
def test_properties(game):
    A, S = MC.SHAPE[game][3:]
    rec = MC.dict_loop_input(game, seed=8)
    rec["n_children"][[17, 200]] = S + 1, 2 ** 32 - 1
    merged = merge_records_host(game, rec)
    group, rep, count, zsum, total, visits = merged
    n, bad = len(rec), int((group < 0).sum())
    assert bad == 2 and group[17] == group[200] == -1 and int(count.sum()) + bad == n
    good = group >= 0
    assert int(zsum.sum()) == int(rec["z"][good].astype(np.int64).sum())
    assert int(total.sum()) == int(rec["total"][good].astype(np.uint64).sum())
    assert np.array_equal(visits.sum(axis=0), rec["visits"][good][:, :A].astype(np.uint64).sum(axis=0))
    assert (np.diff(rep) > 0).all() and np.array_equal(group[rep], np.arange(len(rep)))
    assert np.array_equal(np.bincount(group[good], minlength=len(rep)), count)
    for g in range(len(rep)):  # every member of a group has its representative's key, and none comes before it
        members = np.flatnonzero(group == g)
        assert members[0] == rep[g] and len({MC.key_of(rec[i]) for i in members}) == 1
    assert len({MC.key_of(rec[r]) for r in rep}) == len(rep)
    # permuting the records permutes nothing but rep and the numbering
    perm = np.random.RandomState(1).permutation(n)
    again = merge_records_host(game, rec[perm])
    assert _by_key(rec[perm], again) == _by_key(rec, merged)
    assert np.array_equal(again[0] < 0, (group < 0)[perm]) and (np.diff(again[1]) > 0).all()
    for g in range(len(rep)):
        assert {MC.key_of(r) for r in rec[perm][again[0] == g]} == {MC.key_of(rec[perm][again[1][g]])}


@pytest.mark.parametrize("game", GAMES)
def test_no_duplicates_gives_groups_of_one(game):
    rec = MC.playout_records(game, 120, 2, distinct=True)
    group, rep, count, zsum, total, visits = merge_records_host(game, rec)
    A = MC.SHAPE[game][3]
    assert (count == 1).all() and np.array_equal(group, np.arange(120)) and np.array_equal(rep, np.arange(120))
    assert np.array_equal(zsum, rec["z"]) and np.array_equal(total, rec["total"]) and np.array_equal(visits, rec["visits"][:, :A])
    none = merge_records_host(game, rec[:0])
    assert [len(x) for x in none] == [0] * 6 and none[5].shape == (0, A)


def test_entry_points_check_their_arguments_before_any_device_call():
    for name in ("bb_examples_merge_workspace", "bb_examples_merge", "bb_examples_merged_to_batch"):
        assert name in _lib.EXPORTS
    for game in GAMES:
        assert _lib.examples_merge_workspace(game, 0) == 0
        sizes = [_lib.examples_merge_workspace(game, n) for n in (1, 67, 1000, 1024, 1025, 150000)]
        assert all(s % 16 == 0 for s in sizes) and sizes == sorted(sizes)
        for n, s in zip((1, 67, 1000, 1024, 1025, 150000), sizes):  # two tables of capacity >= 2 n and a word per record
            cap = 1 << int(np.ceil(np.log2(max(2 * n, 64))))
            assert 2 * 4 * cap + 4 * n <= s <= 2 * 4 * cap + 4 * n + 4 * (n // 256 + 1) + 64, (n, s, cap)
        _lib.examples_merge(game, 0, None)                       # nothing to merge: a no-op, GPU or not
        _lib.examples_merged_to_batch(game, 5, None, 3, None, None, None, None, None, 0)
        with pytest.raises(ValueError):
            _lib.examples_merge_workspace(game, -1)
        with pytest.raises(ValueError):
            _lib.examples_merge(game, -1, None)
        with pytest.raises(ValueError):
            _lib.examples_merge(game, 5, None)                   # null records and outputs
        with pytest.raises(ValueError):
            _lib.examples_merge(game, 5, 4096, group=4096, rep=4096, count=4096, zsum=4096, total=4096, visits=4096, n_groups=4096,
                                bad=4096, workspace=None)        # no workspace
        with pytest.raises(ValueError):
            _lib.examples_merge(game, 5, 4096, group=4096, rep=4096, count=4096, zsum=4096, total=4096, visits=4096, n_groups=4096,
                                bad=4096, workspace=4096, workspace_bytes=16)   # too small a workspace
        with pytest.raises(ValueError):
            _lib.examples_merged_to_batch(game, 5, None, 3, None, None, None, None, None, 2)
        with pytest.raises(ValueError):
            _lib.examples_merged_to_batch(game, 5, 4096, 3, 4096, 4096, 4096, 4096, 4096, -1)
    for game in (DC, 7):
        with pytest.raises(ValueError):
            _lib.examples_merge_workspace(game, 10)
        with pytest.raises(ValueError):
            _lib.examples_merge(game, 0, None)
        with pytest.raises(ValueError):
            _lib.examples_merged_to_batch(game, 0, None, 0, None, None, None, None, None, 0)
    assert "DragonChess" in _lib.last_error() or "unknown game" in _lib.last_error()


@pytest.mark.parametrize("game", GAMES)
def test_merged_examples_of_host_records(game):
    """records on the CPU: the host statement is what merged() holds; forming a batch still needs the GPU and says so"""
    S = MC.SHAPE[game][4]
    rec = MC.dict_loop_input(game, seed=5)
    rec["n_children"][3] = S + 1
    ex = DeviceExamples.from_records(game, rec, "cpu")
    m = ex.merged()
    want = merge_records_host(game, rec)
    assert isinstance(m, MergedExamples) and len(m) == len(want[1]) < len(ex) and m.bad() == 1 and m.symmetries == ex.symmetries
    MC.same_merge([t.numpy() for t in (m.group, m.rep, m.count, m.zsum, m.total, m.visits)], want)
    assert np.array_equal(m.counts().numpy(), want[2])
    gi = _lib.game_info(game)
    boards, value, policy = m.batch(np.zeros(0, dtype=np.int64), sym=[])
    assert boards.shape == (0, gi.H, gi.W, gi.C) and value.shape == (0,) and policy.shape == (0, gi.A)
    for wrong in ([len(m)], [-1], torch.tensor([0, len(m)])):   # the range is the number of groups, not of records
        with pytest.raises(IndexError):
            m.batch(wrong)
    with pytest.raises(ValueError):
        m.batch([0, 1], sym=[0, m.symmetries])
    with pytest.raises(ValueError):
        m.batch([0, 1], sym=[0])
    with pytest.raises(_lib.BlackbirdHipError):
        m.batch([0, 1])
    empty = DeviceExamples(game, torch.zeros((0, gi.example_bytes), dtype=torch.uint8)).merged()
    assert len(empty) == 0 and empty.bad() == 0


def test_dragonchess_is_refused_before_any_device_call(tmp_path, monkeypatch):
    from blackbird_amd import Blackbird, DragonChess
    monkeypatch.chdir(tmp_path)

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    for name in ("examples_merge", "examples_merged_to_batch", "examples_to_batch_sym", "examples_to_batch", "Engine"):
        monkeypatch.setattr(_lib, name, no_device)
    ex = DeviceExamples.from_records(DC, np.zeros(4, dtype=_lib.example_dtype(DC)), "cpu")
    with pytest.raises(ValueError, match="DragonChess"):
        ex.merged()
    with pytest.raises(ValueError, match="DragonChess"):
        merge_records_host(DC, np.zeros(4, dtype=_lib.example_dtype(DC)))
    cfg = {"blocks": 1, "filters": 16, "eval": {"dense": 16}, "hasTeacher": False,
           "policy": {"dirichlet": {"alpha": 0.2, "epsilon": 0.3}}, "training": {"optimizer": "adam"}}
    m = Blackbird.Model(DragonChess.BoardState, "dc", {"explorationRate": 0.85, "playLimit": 4}, cfg)
    monkeypatch.setattr(m, "_trainer_for", no_device)
    state = np.random.get_state()
    for examples in (ex, None):
        with pytest.raises(ValueError, match="DragonChess"):
            Blackbird.TrainWithDeviceExamples(m, 2, 0.01, examples=examples, merge=True)
    assert m.Version == 1 and np.array_equal(np.random.get_state()[1], state[1])  # nothing trained, nothing drawn
    m.Conn.Close()
