"""The cases of tests/test_gpu_gnet_envelope.py, checked on the reference alone (no GPU): the rescalings leave the float64
statement alone, the contribution cases separate the six-product kernel model from every one-product and one-plane mutant by a
hundred GPU tolerances, the envelope cases have live heads on the float32 oracle with the first seed that makes them so, and the
extreme cases reach the corners they are named after."""
import functools

import numpy as np
import pytest

from blackbird_amd import _lib, weights as W
from tests import split_cases as S

C4, DC = S.C4, S.DC


def _rel(a, b):
    """the project's metric: relative to max(1, |reference|)"""
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)))


# ---- helpers preserve the function ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game,F,R", S.ENVELOPE_SHAPES + [S.FUSED_SHAPE], ids=lambda x: str(x))
def test_rescalings_leave_the_float64_statement_alone(game, F, R):
    rng = np.random.RandomState(1)
    gi = _lib.game_info(game)
    planes = rng.randint(-1, 2, size=(3, gi.H, gi.W, gi.C)).astype(np.int8)
    w = S.envelope_weights(game, F, R)
    v0, l0 = S._forward64(w, planes)
    assert np.abs(l0).max() > 1e-3 and np.abs(v0).max() > 1e-6
    for name, wc, kind in S.envelope_cases(w, R, wide=F != 16):
        if kind in ("bits", "subnormal"):
            v, l = S._forward64(wc, planes)
            assert _rel(v, v0) <= 1e-12 and _rel(l, l0) <= 1e-12, name
    # and they do rescale: the tensor between the two convolutions of block 0 is 2^-20 of itself
    a0 = S._forward64(w, planes, intermediates=True)[2]
    a1 = S._forward64(S.rescaled_activation(w, 0, 20), planes, intermediates=True)[2]
    assert len(a0) == 2 * R + 1 and a0[1].max() > 0 and np.allclose(a1[1] * 2.0 ** 20, a0[1], rtol=1e-12, atol=0)
    assert np.allclose(a1[2], a0[2], rtol=1e-9, atol=1e-12)


# ---- the contribution cases separate the kernel from its mutants ----------------------------------------------------------------
def test_the_case_list_covers_what_it_claims():
    cases = S.CONTRIBUTION_CASES
    assert len(cases) == len(set(cases)) == 9 * (3 + 3 + 2)
    for game, F, R in S.CONTRIBUTION_SHAPES:
        mine = [c for c in cases if c[:3] == (game, F, R)]
        assert {(c[3], c[4]) for c in mine} == {(l, t) for l in {1, 2, 2 * R} for t in range(9)}  # every tap at every layer
        assert {c[5] for c in mine} == set(S.CHANNELS(F)) and {c[6] for c in mine} == set(S.FILTERS(F))
        assert F % 64 in (16, 48) and F // 16 % 4 in (1, 3)  # a last group of filter blocks that is partly live
    assert {c[:3] for c in cases} == set(S.CONTRIBUTION_SHAPES)


def test_weight_and_activation_have_one_bit_in_each_plane():
    for x in (S.A_IN, S.WV):
        planes = S._widen(S.split3(np.array([x], dtype=np.float32)))[:, 0].astype(np.float64)
        assert planes.sum() == x and all(np.frexp(p)[0] == 0.5 for p in planes), x
    g, v = np.float32(S.BN_ID_GAMMA), np.float32(S.BN_ID_VARIANCE)
    assert g / np.sqrt(v + np.float32(1e-3)) == np.float32(1)       # the float32 forms' scale
    assert abs(float(g) / np.sqrt(float(v) + 1e-3) - 1) < 1e-12     # the statement's


@pytest.mark.parametrize("case", S.CONTRIBUTION_CASES, ids=S.contribution_id)
def test_contribution_case_separates_the_kernel_model_from_every_mutant(case):
    """The statement is unsaturated; the kernel model is 6.5e-7 from it (the three products the form drops, behind the heads' gain:
    split_cases.contribution_network says why that cannot be smaller at this separation) and so inside the GPU tolerance; every
    mutant is at least 100 tolerances away.  Dropping w1.x3 from KERNEL_PRODUCTS makes the second assertion fail."""
    w, info = S.contribution_network(case)
    _st, planes = S.empty_board(case[0])
    v64, l64 = S._forward64(w, planes)
    den = np.maximum(1.0, np.abs(l64))
    dist = lambda out: max(float(np.abs(out[0] - v64).max()), float((np.abs(out[1] - l64) / den).max()))
    assert np.abs(v64).max() < 0.9 and 1 <= np.abs(l64).max() < 2
    model = dist(S.forward_split(w, planes))
    assert model <= 0.66 * S.GPU_TOL, (model, info)
    for name, products in S.mutants().items():
        d = dist(S.forward_split(w, planes, products))
        assert d >= S.SEPARATION * S.GPU_TOL, (name, d, info)


def test_kernel_model_is_the_six_products():
    assert len(S.KERNEL_PRODUCTS) == 6 and all(qw + qx <= 2 for qw, qx in S.KERNEL_PRODUCTS)
    assert len(S.mutants()) == 12
    # on random operands the model is as close to the float64 convolution as three planes allow: 2^-24 of the operands' product
    rng = np.random.RandomState(2)
    t, k = rng.randn(2, 5, 4, 8), rng.randn(3, 3, 8, 6).astype(np.float32)
    b = np.zeros(6, dtype=np.float32)
    exact = S._conv64(t.astype(np.float32).astype(np.float64), k, b)
    assert np.abs(S.split_conv(S.KERNEL_PRODUCTS)(t, k, b) - exact).max() < 72 * 16 * 2.0 ** -24
    assert np.abs(S.split_conv([(0, 0)])(t, k, b) - exact).max() > 1e-3


# ---- the envelope cases ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _envelope_planes(orc, game, F):
    st, idx = S.envelope_positions(game, F)
    return S.oracle_planes(orc, game, st[idx])


def _all_live(orc, game, F, R, seed):
    gi = _lib.game_info(game)
    planes = _envelope_planes(orc, game, F)
    for name, wc, kind in S.envelope_cases(S.envelope_weights(game, F, R, seed), R, wide=F != 16):
        v, l, _p = orc.net_forward(orc.NetWeights(gi.H, gi.W, gi.C, F, R, 16, gi.A, W.flatten(wc)), planes)
        if not S.case_is_live(kind, v, l):
            return False
    return True


@pytest.mark.parametrize("game,F,R", S.ENVELOPE_SHAPES + [S.FUSED_SHAPE], ids=lambda x: str(x))
def test_envelope_cases_are_live_with_the_first_seed_that_makes_them_so(orc, game, F, R):
    """np.ptp(v) >= 0.05, |v|.max() < 0.999 and np.ptp(l, axis=0).max() >= 0.3 on the oracle for every case (the large-activation
    case: the logits alone, its tanh is saturated with every seed), and no seed from 21 up to the chosen one does that."""
    seed = S.ENVELOPE_SEEDS[game, F]
    assert _all_live(orc, game, F, R, seed)
    assert not any(_all_live(orc, game, F, R, s) for s in range(21, seed))


@pytest.mark.parametrize("game,F,R", S.ENVELOPE_SHAPES + [S.FUSED_SHAPE], ids=lambda x: str(x))
def test_extreme_cases_reach_what_they_claim(orc, game, F, R):
    planes = _envelope_planes(orc, game, F)
    w = S.envelope_weights(game, F, R)
    cases = {name: wc for name, wc, _kind in S.envelope_cases(w, R, wide=F != 16)}
    acts = lambda wc: S._forward64(wc, planes, intermediates=True)[2]
    # third plane of the activation subnormal: the tensor between the convolutions of block 0
    u = acts(cases["block 0 activation x 2^-112 (third activation plane subnormal)"])[1].astype(np.float32)
    p = np.abs(S._widen(S.split3(u[u != 0])).astype(np.float64))
    corner = (p[2] < S.BF16_MIN_NORMAL) & (p[2] > 0) & (p[0] >= S.BF16_MIN_NORMAL)
    assert corner.mean() >= 0.5, corner.mean()
    # large k: neither the scaled tensor nor the scaled kernel comes within 2^10 of bf16's largest finite value
    for name, wc in cases.items():
        if "activation x" in name:
            block = int(name.split()[1])
            top = max(acts(wc)[2 * block + 1].max(), np.abs(wc[f"resTower/block_{block}/conv_2/kernel"]).max())
            assert 0 < top <= S.BF16_MAX / 2.0 ** 10, (name, top)
    if F != 16:
        assert max(a.max() for a in acts(cases["variance 1e-8, gamma x 64"])) > 1e4
        k = cases["layer 1 x 2^-112 (third weight plane subnormal)"]["resTower/block_0/conv_1/kernel"]
        p = np.abs(S._widen(S.split3(k[k != 0])).astype(np.float64))
        assert ((p[2] < S.BF16_MIN_NORMAL) & (p[0] >= S.BF16_MIN_NORMAL)).mean() >= 0.5  # (most of them below bf16's last subnormal bit)
