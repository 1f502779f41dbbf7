"""-m gpu: the BATCH launch of the launch-per-layer network (gnet.hip.h, gnet_x3.hip.h, launch_gnet in host_weights.hip.h) for every
game, width and form.

launch_gnet cuts a call one of two ways: one position x one filter block per wave (small launch), or PPB positions x FBW
filter blocks per wave (batch launch: every larger call and every self-play round).  Both run the same K order per output, so
they must give the same bits.  Engine.net_eval_structure(n) says which of the two a call of n positions takes; every case here
asserts the launch it means to run instead of restating the engine's threshold.

What the shapes reach (NCB = F / 16 filter blocks; a wave of the batch launch holds FBW = 2 of them in the float32-MFMA
kernel k_gnet_conv and 4 in the split-form kernel k_gnet_conv_x3; the four waves of a workgroup take `per` = 1, 2 or 4
neighbouring groups of FBW blocks):
  * a last wave that holds 1, 2 or 3 live blocks of its FBW (computed on block NCB - 1, not stored), and a wave that leaves
    because its first block is past NCB;
  * per = 1, 2 and 4 in either form;
  * a last group of PPB positions that holds exactly one position, or all but one (valid[t]);
  * the tile geometry of every game: Connect4 packs 4 positions into 10.5 of 11 tiles, TicTacToe 16 positions into 9 tiles
    (every tile straddles positions), DragonChess 2 positions into 8 tiles; DragonChess is also the game whose input planes
    are padded (17 -> 20) and whose policy head is 4032 wide."""
import functools

import numpy as np
import pytest

from blackbird_amd import _lib, weights as W
from tests.net_cases import TOL, errors, eval_forms, positions, selfplay_vs_oracle_tree

pytestmark = pytest.mark.gpu
C4, TTT, DC = _lib.GAME_CONNECT4, _lib.GAME_TICTACTOE, _lib.GAME_DRAGONCHESS
GAME_IDS = {C4: "c4", TTT: "ttt", DC: "dc"}
PPB = {C4: 4, TTT: 16, DC: 2}  # GNetGeom<G>::PPB: the positions a wave of the batch launch holds
FORMS = [_lib.NET_FORM_AUTO, _lib.NET_FORM_F32]
FORM_IDS = ["split", "f32"]
OUTPUTS = ("value", "logits", "policy")

# (F, R, {game: n}): n is the smallest batch that takes the batch launch and leaves exactly one position in the last group
ROWS = [(32, 2, {C4: 1025, TTT: 1025, DC: 1025}),   # split: the wave holds 2 of 4 blocks
        (48, 1, {C4: 685, TTT: 689, DC: 683}),      # split: 3 of 4; float32: the second wave holds 1 of 2
        (80, 2, {C4: 413, TTT: 417, DC: 411}),      # split: 4 + 1 of 4; float32: grid.y = 2 and a wave that leaves at fb0 >= NCB
        (96, 1, {C4: 345, TTT: 353, DC: 343}),      # split: 4 + 2 of 4
        (144, 1, {C4: 229, TTT: 241, DC: 229}),     # split: 3 groups of blocks, per = 2, the last wave leaves; float32: per = 4
        (256, 1, {C4: 129, TTT: 129, DC: 129})]     # per = 4 in both forms
CASES = [(g, F, R, ns[g]) for F, R, ns in ROWS for g in (C4, TTT, DC)]
RAGGED = [(C4, 32, 2, 1027), (TTT, 32, 2, 1039)]    # n % PPB == PPB - 1: the last group lacks one position
# The value head is ONE channel behind a ReLU and the policy head two: with most random weights one of them is dead or its tanh
# saturated on every position, and the outputs then say nothing about the tower.  Per (game, F) the first init_weights seed
# from 21 up with which the oracle's value and logits both move with the position (_reference asserts by how much).
SEEDS = {(C4, 32): 22, (TTT, 32): 22, (DC, 32): 24, (C4, 48): 23, (TTT, 48): 27, (DC, 48): 21, (C4, 80): 27, (TTT, 80): 23,
         (DC, 80): 63, (C4, 96): 30, (TTT, 96): 27, (DC, 96): 51, (C4, 144): 23, (TTT, 144): 23, (DC, 144): 32,
         (C4, 256): 77, (TTT, 256): 25, (DC, 256): 54}


def _ids(cases):
    return [f"{GAME_IDS[g]}-F{F}-R{R}-n{n}" for g, F, R, n in cases]


@functools.lru_cache(maxsize=None)
def _case(game, F, R, n):
    """weights, positions and their planes for one (game, shape, batch): made once, shared by the forms, never changed"""
    gi = _lib.game_info(game)
    flat = W.flatten(W.init_weights(gi.C, F, R, 16, gi.A, seed=SEEDS[game, F], perturb=True))
    st = positions(game, n, seed=F + n)
    return flat, st, _lib.game_encode(game, st)


def _oracle_subset(game, n):
    """The positions the oracle sees: the first two groups of PPB positions, the two groups either side of a workgroup boundary
    near the middle, and the last two groups (the ragged one included).  Four groups are a whole number of workgroups for every
    cut of the four waves (per = 1, 2, 4: 4, 2, 1 groups a workgroup) and of k_gnet_heads (4 positions a workgroup).
    Connect4: 21 positions, DragonChess: 11; TicTacToe: 81 (its groups are 16 positions of 9 cells: fewer cells than Connect4's)."""
    ppb = PPB[game]
    groups = (n + ppb - 1) // ppb
    mid = groups // 2 // 4 * 4
    assert 2 <= mid - 1 and mid <= groups - 3, (n, groups)
    idx = [i for g in (0, 1, mid - 1, mid, groups - 2, groups - 1) for i in range(g * ppb, min((g + 1) * ppb, n))]
    assert idx[-1] == n - 1 and len(set(idx)) == len(idx)
    return np.array(idx)


@functools.lru_cache(maxsize=None)
def _reference(orc, game, F, R, n):
    flat, _st, planes = _case(game, F, R, n)
    gi = _lib.game_info(game)
    ref = orc.net_forward(orc.NetWeights(gi.H, gi.W, gi.C, F, R, 16, gi.A, flat), planes[_oracle_subset(game, n)])
    v, l, _p = ref
    # a property of the chosen weights and positions, asserted on the oracle alone: both heads are live and see the position
    assert np.ptp(v) >= 0.05 and np.abs(v).max() < 0.999 and np.ptp(l, axis=0).max() >= 0.3, (game, F, R, n)
    return ref


def _engine(game, form, flat, R):
    eng = _lib.Engine(game, n_slots=4, sims_per_move=2, evaluator=_lib.EVAL_NET, max_plies=8 if game == DC else None, net_form=form)
    try:
        eng.load_weights(flat)
        assert eng.net_form() == (3 if form != _lib.NET_FORM_F32 and R > 0 else 1)
    except BaseException:
        eng.close()
        raise
    return eng


def _small_chunk(eng):
    """a batch size the engine runs as a small launch, asked of the engine"""
    chunk = 128
    while chunk > 1 and eng.net_eval_structure(chunk) != _lib.NET_EVAL_SMALL:
        chunk //= 2
    assert eng.net_eval_structure(chunk) == _lib.NET_EVAL_SMALL
    return chunk


def test_net_eval_structure_answers_and_refusals():
    """bb_net_eval_structure: BB_ERR_WEIGHTS before bb_load_weights, BB_ERR_ARG on a null argument or a negative n, the fused
    tower for a 16-filter network, and for a wide one the small launch for one position and the batch launch for very many."""
    import ctypes
    L = _lib.lib()
    out = ctypes.c_int32(-1)
    gi = _lib.game_info(C4)
    eng = _lib.Engine(C4, n_slots=4, sims_per_move=2, evaluator=_lib.EVAL_NET)
    try:
        assert L.bb_net_eval_structure(eng.h, 1, ctypes.byref(out)) == _lib.ERR_WEIGHTS and out.value == -1
        eng.load_weights(W.flatten(W.init_weights(gi.C, 16, 1, 16, gi.A, seed=1)))
        assert [eng.net_eval_structure(n) for n in (0, 1, 1 << 20)] == [_lib.NET_EVAL_FUSED] * 3
        eng.load_weights(W.flatten(W.init_weights(gi.C, 32, 1, 16, gi.A, seed=1)))
        assert eng.net_eval_structure(1) == _lib.NET_EVAL_SMALL and eng.net_eval_structure(1 << 20) == _lib.NET_EVAL_BATCH
        assert L.bb_net_eval_structure(eng.h, -1, ctypes.byref(out)) == _lib.ERR_ARG
        assert L.bb_net_eval_structure(eng.h, 1, None) == _lib.ERR_ARG
        assert L.bb_net_eval_structure(None, 1, ctypes.byref(out)) == _lib.ERR_ARG
        with pytest.raises(ValueError):
            eng.net_eval_structure(-1)
    finally:
        eng.close()


def _same_bits(got, want, what):
    for a, b, name in zip(got, want, OUTPUTS):
        if not np.array_equal(a, b):
            bad = np.unique(np.nonzero(a != b)[0])
            raise AssertionError(f"{what}: {name} differs at {len(bad)} of {len(a)} positions, first {bad[:8]}, last {bad[-1]}")


def _check_batch(orc, game, form, F, R, n, last):
    flat, st, planes = _case(game, F, R, n)
    what = f"gnet-batch {GAME_IDS[game]} {FORM_IDS[FORMS.index(form)]} F{F} R{R} n{n}"
    assert n % PPB[game] == last
    eng = _engine(game, form, flat, R)
    try:
        # 1. one batch call
        assert eng.net_eval_structure(n) == _lib.NET_EVAL_BATCH
        got = eng.net_eval(states=st)
        # 2. the same positions through the small launch: identical bits, every position
        chunk = _small_chunk(eng)
        for lo in range(0, n, chunk):
            part = st[lo:lo + chunk]
            assert eng.net_eval_structure(len(part)) == _lib.NET_EVAL_SMALL
            _same_bits(eng.net_eval(states=part), tuple(a[lo:lo + chunk] for a in got), f"{what}: small launch of {lo}..")
        # 3. planes input: k_gnet_input's other branch at batch size
        _same_bits(eng.net_eval(planes=planes), got, what + ": planes")
        # 4. the oracle
        idx = _oracle_subset(game, n)
        ref = _reference(orc, game, F, R, n)
        sub = tuple(a[idx] for a in got)
        ev, el, ep = errors(sub, ref)
        exact = float(np.mean(sub[1] == ref[1]))
        print(f"{what}: value {ev:.2e} logits {el:.2e} policy {ep:.2e} ({len(idx)} positions; logits bit-equal {exact:.4f})")
        assert ev <= TOL and el <= TOL and ep <= TOL, what
        if form == _lib.NET_FORM_F32:  # the float32-MFMA layers are the oracle's fmaf chains
            if game == DC:
                assert np.array_equal(sub[0], ref[0]) or ev <= 2e-7, what
            else:
                assert exact > 0.99, what
        # 5. a permutation of the batch: permuted bits
        perm = np.random.RandomState(n + F).permutation(n)
        _same_bits(eng.net_eval(states=st[perm]), tuple(a[perm] for a in got), what + ": permuted")
    finally:
        eng.close()


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("game,F,R,n", CASES, ids=_ids(CASES))
def test_batch_launch_equals_small_launch_and_oracle(orc, game, F, R, n, form):
    """One batch-launch call against the same positions in small-launch chunks (identical bits), against planes input (identical
    bits), against the oracle on the first, middle and last groups (1e-5; float32 form: the oracle's own K order) and against a
    permutation of itself (permuted bits).  The last group of every batch holds one position."""
    _check_batch(orc, game, form, F, R, n, last=1)


@pytest.mark.parametrize("game,F,R,n", RAGGED, ids=_ids(RAGGED))
def test_batch_launch_with_a_last_group_short_of_one_position(orc, game, F, R, n):
    """the other raggedness: n % PPB == PPB - 1 (a TicTacToe tile then ends inside the one missing position)"""
    _check_batch(orc, game, _lib.NET_FORM_AUTO, F, R, n, last=PPB[game] - 1)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("game", [C4, TTT, DC], ids=["c4", "ttt", "dc"])
def test_nothing_leaks_between_calls_on_one_engine(game, form):
    """Batch A, batch B (other positions), a small launch, batch A again -- on ONE engine.  The zero halo ring of the activation
    buffers is written once, at allocation: a lane that stored where valid[t] is false, or for a padded tile column, would change
    what a later call reads.  The second A equals the first, and every stage equals a fresh engine's bits."""
    F, R = 48, 1
    n_a = ROWS[1][2][game]
    flat, st_a, _planes = _case(game, F, R, n_a)
    eng = _engine(game, form, flat, R)
    try:
        n_b = 1  # the smallest batch-launch size with one position in the last group, asked of the engine
        while eng.net_eval_structure(n_b) != _lib.NET_EVAL_BATCH or n_b % PPB[game] != 1:
            n_b += 1
            assert n_b < 1 << 16
        stages = [("A", st_a, _lib.NET_EVAL_BATCH), ("B", positions(game, n_b, seed=7), _lib.NET_EVAL_BATCH),
                  ("small", positions(game, 37, seed=8), _lib.NET_EVAL_SMALL), ("A again", st_a, _lib.NET_EVAL_BATCH)]
        outs = []
        for name, st, structure in stages:
            assert eng.net_eval_structure(len(st)) == structure, name
            outs.append(eng.net_eval(states=st))
    finally:
        eng.close()
    _same_bits(outs[3], outs[0], "A again")
    for (name, st, _structure), out in zip(stages[:3], outs):
        fresh = _engine(game, form, flat, R)
        try:
            _same_bits(out, fresh.net_eval(states=st), name + " against a fresh engine")
        finally:
            fresh.close()


DC_WIDE = [(32, 0, 16), (32, 2, 1), (32, 2, 17), (32, 2, 64), (48, 1, 16)]  # (F, R, D)


@pytest.mark.parametrize("F,R,D", DC_WIDE, ids=[f"F{F}-R{R}-D{D}" for F, R, D in DC_WIDE])
def test_dragonchess_behind_a_wide_tower(orc, F, R, D):
    """DragonChess (17 planes padded to 20, the 4032-wide policy head of k_gnet_heads) through the small launch over block count
    and value-head width, 7 positions and 1, in both forms, against the oracle; a position alone gives the same bits."""
    gi = _lib.game_info(DC)
    flat = W.flatten(W.init_weights(gi.C, F, R, D, gi.A, seed=13, perturb=True))
    forms = [("split", {}, 3 if R else 1), ("f32", dict(net_form=_lib.NET_FORM_F32), 1)]
    eval_forms(orc, DC, flat, forms, positions(DC, 7, seed=100 * R + D))


def test_tictactoe_selfplay_with_a_wide_network_matches_oracle_tree(orc):
    """Asynchronous rounds take the batch size from the device: the batch launch of the TicTacToe instantiation at whatever the
    rounds' leaf lists hold (21 slots: ragged groups of 16).  The oracle's search, fed the GPU network's values, plays the same
    games."""
    selfplay_vs_oracle_tree(orc, filters=32, blocks=2, game=TTT, og=1, n_slots=21, n_games=30, sims=16, max_plies=10)
