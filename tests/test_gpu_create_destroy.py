"""-m gpu: create and destroy give back what they took (csrc/dev_mem.h: every engine, arena and trainer has one owner of its device
memory, streams and events).

One warm-up cycle of create, one small call, destroy -- the runtime's own first-use allocations happen there --, then the device's
free memory is read, ten more cycles run, and it is read again: it must not have fallen by as much as ONE object's own
footprint, so a leak of one cycle in ten would show.  The footprints: an engine's is n_slots * bytes_per_slot (bb_fit_slots) plus
its example store; a trainer's the sum trainer_alloc checks against the free memory, (max_batch + 8) parameter arrays; an arena's
the 17 per-slot arrays of ArenaDev (csrc/arena.hip.h: the state, eight bytes and seven words per slot), next to which the two
engines it plays are large.  The shapes are the smallest the API admits.  A create call refused for a bad argument leaves free
memory as it was: bb_create's check of `launch` comes after its stream and events exist.  Nothing here exhausts memory or makes a
HIP call fail.

What this reading can see: on the MI355X the runtime takes small allocations out of 2 MiB blocks of its own, and the device's free
memory moved in such steps when this was written (every figure below was equal before and after the ten cycles), so a leak shows
here once it has used up the block in hand -- the exact count, allocation by allocation and for every failing call of a create
function, is tests/test_dev_mem_cpu.py's, over a heap that counts."""
import ctypes as C

import numpy as np
import pytest
import torch

from blackbird_amd import _lib
from blackbird_amd import weights as W

pytestmark = pytest.mark.gpu
CYCLES = 10


def _free():
    torch.cuda.synchronize(0)
    return torch.cuda.mem_get_info(0)[0]


def _engine(game, **kw):
    return _lib.Engine(game, n_slots=2, sims_per_move=4, evaluator=_lib.EVAL_HASH, hash_salt=3, seed=1, **kw)


def _engine_bytes(game):
    info = _lib.game_info(game)
    max_plies = {_lib.GAME_CONNECT4: 42, _lib.GAME_TICTACTOE: 9}[game]
    fit, per_slot = _lib.fit_slots(game, 2, 4)
    assert fit == 2
    return 2 * per_slot + 2 * (max_plies + 1) * info.example_bytes


def _engine_cycle(game):
    eng = _engine(game)
    states = np.concatenate([_lib.game_initial(game)] * 2)
    eng.set_roots(states)
    eng.run_sims(2)
    eng.run_sims(2, mask=[1, 1])  # (the mask is staged on the device)
    assert eng.root_states().tobytes() == states.tobytes()
    eng.close()


def _arena_cycle(game):
    a, b = _engine(game), _engine(game)
    ar = _lib.Arena(a, b, log_plies=4)
    ar.begin(np.array([1, 0], dtype=np.uint8), 0.0)
    ar.step(1)
    assert ar.status() == 2
    ar.close()
    a.close()
    b.close()


def _trainer_flat(game):
    info = _lib.game_info(game)
    return info, W.flatten(W.init_weights(info.C, 16, 0, 16, info.A, seed=2))


def _trainer_cycle(game):
    info, flat = _trainer_flat(game)
    h = _lib.trainer_create(game, flat, info.H, info.W, _lib.OPT_ADAM, 2)
    n = _lib.trainer_param_count(h)
    assert _lib.trainer_read(h, _lib.TRAIN_PARAMS).shape == (n,)
    _lib.trainer_destroy(h)
    return n


def _cycles_keep_free_memory(cycle, footprint, what):
    cycle()  # warm-up
    before = _free()
    for _ in range(CYCLES):
        cycle()
    after = _free()
    print(f"{what}: free memory {before} -> {after} after {CYCLES} cycles, one object's footprint {footprint} bytes")
    assert footprint > 0 and before - after < footprint, (what, before, after, footprint)


@pytest.mark.parametrize("game", [_lib.GAME_TICTACTOE, _lib.GAME_CONNECT4])
def test_engine_cycles_give_their_memory_back(game):
    _cycles_keep_free_memory(lambda: _engine_cycle(game), _engine_bytes(game), f"engine of game {game}")


@pytest.mark.parametrize("game", [_lib.GAME_TICTACTOE, _lib.GAME_CONNECT4])
def test_arena_cycles_give_their_memory_back(game):
    info = _lib.game_info(game)
    arena_bytes = 2 * (info.state_bytes + 8 + 7 * 4 + 4 * 4)  # per slot: the state, 8 byte arrays, 7 word arrays, log_plies = 4 words
    _cycles_keep_free_memory(lambda: _arena_cycle(game), arena_bytes, f"arena over two engines of game {game}")


@pytest.mark.parametrize("game", [_lib.GAME_TICTACTOE, _lib.GAME_CONNECT4])
def test_trainer_cycles_give_their_memory_back(game):
    params = _trainer_cycle(game)
    _cycles_keep_free_memory(lambda: _trainer_cycle(game), (2 + 8) * params * 4, f"trainer of game {game} (R = 0, max_batch 2)")


def test_refused_creates_leave_free_memory_unchanged():
    game = _lib.GAME_TICTACTOE
    _engine_cycle(game)
    _trainer_cycle(game)
    info, flat = _trainer_flat(game)
    before = _free()
    for _ in range(CYCLES):
        with pytest.raises(ValueError, match="launch"):
            _engine(game, launch=99)  # refused after the engine's stream and events were made
        with pytest.raises(ValueError, match="optimizer"):
            _lib.trainer_create(game, flat, info.H, info.W, 99, 2)
    after = _free()
    print(f"refused creates: free memory {before} -> {after}")
    assert after == before
    h = C.c_void_p(1)
    cfg = _lib.TrainConfig(game=int(game), optimizer=99, max_batch=2, device=0, momentum=0.9, alpha=0.2, epsilon=0.3, seed=0)
    w, _keep = _lib.net_weights(info.H, info.W, flat)
    assert _lib.lib().bb_trainer_create(C.byref(cfg), C.byref(w), C.byref(h)) == _lib.ERR_ARG and not h.value  # no handle comes back
