"""-m gpu: the split-operand tower of the launch-per-layer network (k_gnet_conv_x3 in gnet_x3.hip.h, net_form() == 3) over its
arithmetic envelope, through the two launches of bb_net_eval (small and batch); and the activation rescalings on the 16-filter
form (net_x3.hip.h), whose own envelope test scales weights only.

The cases are tests/split_cases.py's; tests/test_split_cases_cpu.py shows without a GPU that they can fail: every lost plane
or product of the contribution cases is a hundred tolerances from the float64 statement, the envelope cases have live heads, the
extreme cases reach their corners."""
import numpy as np
import pytest

from blackbird_amd import _lib, weights as W
from tests import split_cases as S
from tests.net_cases import TOL, oracle_forward
from tests.test_gpu_gnet_batch import ROWS, _engine, _same_bits, _small_chunk

pytestmark = pytest.mark.gpu
C4, TTT, DC = S.C4, S.TTT, S.DC
# e_gpu <= C64 x e_orc against float64 where a third plane is a bf16 subnormal: see test_wide_split_envelope
SUBNORMAL_C64 = 4.0


@pytest.fixture(scope="module")
def engines():
    """one engine per (game, F, R, form), kept across load_weights calls (test_reload_another_shape_on_a_live_engine shows that a
    live engine takes new weights), closed when the module is done"""
    made = {}

    def get(game, F, R, flat, form=_lib.NET_FORM_AUTO):
        if (game, F, R, form) in made:
            made[game, F, R, form].load_weights(flat)
        elif F == 16:
            eng = _lib.Engine(game, n_slots=4, sims_per_move=2, evaluator=_lib.EVAL_NET, net_form=form)
            eng.load_weights(flat)
            made[game, F, R, form] = eng
        else:
            made[game, F, R, form] = _engine(game, form, flat, R)
        eng = made[game, F, R, form]
        assert eng.net_form() == (2 if F == 16 else 3)
        return eng

    yield get
    for eng in made.values():
        eng.close()


def _small(eng, st):
    """st through small launches only"""
    chunk = _small_chunk(eng)
    parts = []
    for lo in range(0, len(st), chunk):
        assert eng.net_eval_structure(len(st[lo:lo + chunk])) == _lib.NET_EVAL_SMALL
        parts.append(eng.net_eval(states=st[lo:lo + chunk]))
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def _batch(eng, st):
    assert eng.net_eval_structure(len(st)) == _lib.NET_EVAL_BATCH
    return eng.net_eval(states=st)


@pytest.mark.parametrize("case", S.CONTRIBUTION_CASES, ids=S.contribution_id)
def test_every_tap_plane_and_channel_block_contributes(engines, case):
    """One weight 1 + 2^-10 + 2^-20 on one (tap, channel, filter) of one tower layer meets the activation 1 + 2^-9 + 2^-18: value
    and logits of the empty board equal the float64 statement within 1e-6 (logits relative to max(1, |logit|)) only if that tap's
    slice of that channel block carried all three planes of both operands through all six products, the layers behind it all
    three planes of the activation, and the heads read the last layer's float32 layout at filter f.  Expected distance: 6.5e-7, the
    three products the form drops by design; any lost plane or product: >= 1e-4 (tests/test_split_cases_cpu.py).  The tap-8 case
    of every layer also goes through the batch launch: the small launch's bits at every position."""
    game, F, R, layer, tap, c, f = case
    w, _info = S.contribution_network(case)
    st, planes = S.empty_board(game)
    assert np.array_equal(_lib.game_encode(game, st), planes)
    eng = engines(game, F, R, W.flatten(w))
    assert eng.net_eval_structure(1) == _lib.NET_EVAL_SMALL
    v, l, p = eng.net_eval(states=st)
    v64, l64 = S._forward64(w, planes)
    ev, el = float(np.abs(v - v64).max()), float((np.abs(l - l64) / np.maximum(1.0, np.abs(l64))).max())
    print(f"{S.contribution_id(case)}: value {ev:.2e} logits {el:.2e}")
    assert ev <= S.GPU_TOL and el <= S.GPU_TOL, (case, ev, el)
    if tap == 8:
        n = next(ns[game] for f_, _r, ns in ROWS if f_ == F)
        got = _batch(eng, np.repeat(st, n, axis=0))
        _same_bits(got, tuple(np.repeat(a, n, axis=0) for a in (v, l, p)), "batch launch")


def _two_sided(orc, game, wts, got, planes, what, tol=TOL, c64=4.0):
    """the rule of test_split_operand_envelope: against the oracle max(tol, 1.25 (e_gpu + e_orc)), against float64
    e_gpu <= max(c64 e_orc, 2e-6); the figures are printed first"""
    v, l, p = got
    ov, ol, op = oracle_forward(orc, game, W.flatten(wts), planes)
    v64, l64 = S._forward64(wts, planes)
    assert np.isfinite(v).all() and np.isfinite(l).all() and np.isfinite(p).all(), what
    den = np.maximum(1.0, np.abs(l64))
    e_gpu, e_orc = np.max(np.abs(l - l64) / den), np.max(np.abs(ol - l64) / den)
    print(f"{what}: |logit| <= {np.abs(l64).max():.3g}; vs oracle {np.max(np.abs(l - ol) / den):.2e}; vs float64: GPU {e_gpu:.2e}, "
          f"oracle {e_orc:.2e}, ratio {e_gpu / e_orc:.2f}")
    tol_l = max(tol, 1.25 * (e_gpu + e_orc))
    assert np.max(np.abs(l - ol) / den) <= tol_l and np.max(np.abs(v - ov)) <= tol_l and np.max(np.abs(p - op)) <= tol_l, what
    assert e_gpu <= max(c64 * e_orc, 2e-6), what  # as accurate as float32 arithmetic itself


@pytest.mark.parametrize("game,F,R", S.ENVELOPE_SHAPES, ids=[f"{S.GAME_IDS[g]}-F{F}-R{R}" for g, F, R in S.ENVELOPE_SHAPES])
def test_wide_split_envelope(orc, engines, game, F, R):
    """test_split_operand_envelope for the wide form, in both launches of bb_net_eval: a ragged batch through the batch launch and
    its first, middle and last groups through the small launch give the same bits in every case, and
      * base: the two-sided rule against the oracle and the float64 statement;
      * a layer's weights (the float32 first convolution that writes the planes, conv_1, conv_2 with the skip, the last layer
        with the float32 layout) times 2^+-20 and 2^+-12, and the stored activation between the convolutions of the first and of
        the last block times 2^+-20: the base's bits;
      * activations beyond 1e4 (variance 1e-8, gamma x 64 on the first two layers): the two-sided rule;
      * a third plane that is a bf16 subnormal, of the weights (layer 1 x 2^-112) and of the stored activations (block 0 x 2^-112,
        which x3_split4 rounds on the device where the weights are split on the host): the two-sided rule with SUBNORMAL_C64.
    Measured on the MI355X (logits; GPU against float64, oracle against float64, ratio): base 1.72e-07 / 1.30e-07 / 1.32
    (Connect4), 1.46e-07 / 1.11e-07 / 1.32 (DragonChess); large activations 2.42e-04 / 9.09e-05 / 2.66 and 1.05e-04 / 6.63e-04 /
    0.16; weights' third plane subnormal 2.80e-07 / 1.30e-07 / 2.15 and 1.27e-06 / 1.11e-07 / 11.4 (under the rule's 2e-6 floor);
    activations' third plane subnormal 1.53e-07 / 1.30e-07 / 1.18 and 1.36e-07 / 1.11e-07 / 1.23.  The factor 4 of every other
    case holds in the subnormal corners too: the wide form needs none of the 16-filter form's 1e-4 and 64."""
    st, idx = S.envelope_positions(game, F)
    planes = _lib.game_encode(game, st[idx])
    base = None
    for what, wts, kind in S.envelope_cases(S.envelope_weights(game, F, R), R):
        eng = engines(game, F, R, W.flatten(wts))
        small = _small(eng, st[idx])
        _same_bits(tuple(a[idx] for a in _batch(eng, st)), small, what + ": batch launch against small launch")
        if kind == "base":
            base = small
            _two_sided(orc, game, wts, small, planes, what)
        elif kind == "bits":  # powers of two scale every plane and every product exactly
            _same_bits(small, base, what + ": against the base")
        elif kind == "two-sided":
            _two_sided(orc, game, wts, small, planes, what)
        else:
            _two_sided(orc, game, wts, small, planes, what, c64=SUBNORMAL_C64)


def test_fused_split_activation_rescaling(orc, engines):
    """The 16-filter form (net_x3.hip.h, NET_FORM_SPLIT) under the activation rescalings its own envelope test leaves out: the
    tensor between the convolutions of the first and the last block times 2^+-20 gives the base's bits; times 2^-112 (third plane
    a bf16 subnormal in LDS) it keeps the two-sided rule."""
    game, F, R = S.FUSED_SHAPE
    st, idx = S.envelope_positions(game, F)
    planes = _lib.game_encode(game, st)
    base = None
    for what, wts, kind in S.envelope_cases(S.envelope_weights(game, F, R), R, wide=False):
        eng = engines(game, F, R, W.flatten(wts), form=_lib.NET_FORM_SPLIT)
        assert eng.net_eval_structure(len(st)) == _lib.NET_EVAL_FUSED
        got = eng.net_eval(states=st)
        if kind == "base":
            base = got
            _two_sided(orc, game, wts, got, planes, what)
        elif kind == "bits":
            _same_bits(got, base, what + ": against the base")
        else:
            _two_sided(orc, game, wts, got, planes, what, c64=SUBNORMAL_C64)
