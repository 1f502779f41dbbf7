"""What the tests of the split-operand towers share (not collected): the float64 statement of the graph, function-preserving
rescalings of a layer's weights and of a stored activation, a numpy model of the three-plane bf16 product with a chosen subset of
its nine plane products, and the two case lists of tests/test_gpu_gnet_envelope.py -- the contribution cases (one weight with a
bit in every plane, on one tap, channel and filter of one layer) and the envelope cases.  tests/test_split_cases_cpu.py shows on
the reference alone that these cases can fail: no GPU is needed for anything here."""
import functools

import numpy as np

from blackbird_amd import _lib, weights as W

F32, U16, U32 = np.float32, np.uint16, np.uint32
C4, TTT, DC = _lib.GAME_CONNECT4, _lib.GAME_TICTACTOE, _lib.GAME_DRAGONCHESS
GAME_IDS = {C4: "c4", TTT: "ttt", DC: "dc"}


# ---- bf16 planes ------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(U32)


def _bf16_nearest(x):
    """float32 -> bf16 bits, round to nearest, ties to even (finite values)"""
    u = _bits(x).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(U16)


def _widen(p):
    return (np.ascontiguousarray(p, dtype=U16).astype(U32) << 16).view(F32)


def split3(x):
    """[3, *x.shape] uint16: plane k is the bf16 nearest (ties to even) to what planes < k leave of the float32 x"""
    x = np.ascontiguousarray(x, dtype=F32)
    p1 = _bf16_nearest(x)
    r = x - _widen(p1)
    p2 = _bf16_nearest(r)
    p3 = _bf16_nearest(r - _widen(p2))
    return np.stack([p1, p2, p3])


BF16_MAX = float(_widen(np.array([0x7F7F], dtype=U16))[0])
BF16_MIN_NORMAL = 2.0 ** -126


# ---- the float64 statement --------------------------------------------------------------------------------------------------
def _conv64(t, k, b):
    kh = k.shape[0] // 2
    tp = np.pad(t, ((0, 0), (kh, kh), (kh, kh), (0, 0)))
    out = np.zeros(t.shape[:3] + (k.shape[3],))
    for dy in range(k.shape[0]):
        for dx in range(k.shape[1]):
            out += np.einsum("nhwc,cf->nhwf", tp[:, dy:dy + t.shape[1], dx:dx + t.shape[2], :], k[dy, dx].astype(np.float64))
    return out + b.astype(np.float64)


def _forward64(w, planes, intermediates=False, tower_conv=None):
    """The graph of NetworkFactory.py:22-183 in float64 numpy (NHWC, SAME padding, batch-norm epsilon 1e-3): an independent
    statement of what both the float32 oracle and the GPU forms approximate.  Returns value, logits; with `intermediates` also
    the list of the tower's activations (entry 0: the first convolution's output, entry l: tower layer l's, after its ReLU;
    for conv_1 of a block that is the tensor between the block's two convolutions).  `tower_conv` replaces the convolution of
    the tower layers 1 .. 2R (the model of the split product below); the statement itself never passes one."""
    x = planes.astype(np.float64)
    conv = _conv64
    tconv = tower_conv or conv

    def bn(t, p):
        g, b, m, v = (w[f"{p}/{n}"].astype(np.float64) for n in ("gamma", "beta", "moving_mean", "moving_variance"))
        return g * (t - m) / np.sqrt(v + 1e-3) + b

    relu = lambda t: np.maximum(t, 0.0)
    t = relu(bn(conv(x, w["resTower/conv_block/conv/kernel"], w["resTower/conv_block/conv/bias"]), "resTower/conv_block/batch_norm"))
    acts = [t]
    i = 0
    while f"resTower/block_{i}/conv_1/kernel" in w:
        u = relu(bn(tconv(t, w[f"resTower/block_{i}/conv_1/kernel"], w[f"resTower/block_{i}/conv_1/bias"]), f"resTower/block_{i}/batch_norm_1"))
        acts.append(u)
        u = bn(tconv(u, w[f"resTower/block_{i}/conv_2/kernel"], w[f"resTower/block_{i}/conv_2/bias"]), f"resTower/block_{i}/batch_norm_2")
        t = relu(u + t)
        acts.append(t)
        i += 1
    v = relu(bn(conv(t, w["value/convolution/kernel"], w["value/convolution/bias"]), "value/batch_norm"))
    v = (v @ w["value/dense_1/kernel"].astype(np.float64) + w["value/dense_1/bias"]).sum(axis=(1, 2))
    v = np.tanh(relu(v) @ w["value/dense_2/kernel"].astype(np.float64) + w["value/dense_2/bias"])[:, 0]
    p = relu(bn(conv(t, w["policy/convolution/kernel"], w["policy/convolution/bias"]), "policy/batch_norm"))
    logits = (p @ w["policy/policy/kernel"].astype(np.float64) + w["policy/policy/bias"]).sum(axis=(1, 2))
    return (v, logits, acts) if intermediates else (v, logits)


# ---- rescalings that leave the network function alone -------------------------------------------------------------------------
def _layer_names(blocks):
    names = [("resTower/conv_block/conv", "resTower/conv_block/batch_norm")]
    for i in range(blocks):
        names += [(f"resTower/block_{i}/conv_{j}", f"resTower/block_{i}/batch_norm_{j}") for j in (1, 2)]
    return names


def _rescaled(w, layer, k, blocks):
    """Kernel, bias and moving mean of one conv layer times 2^k, its batch-norm gamma divided by 2^k: the network function is
    unchanged in exact arithmetic, and every scaling is a power of two -- exact in float32 and in every bf16 plane."""
    conv, bnp = _layer_names(blocks)[layer]
    out = {n: a.copy() for n, a in w.items()}
    s = np.float32(2.0) ** k
    out[conv + "/kernel"] = (w[conv + "/kernel"] * s).astype(np.float32)
    out[conv + "/bias"] = (w[conv + "/bias"] * s).astype(np.float32)
    out[bnp + "/moving_mean"] = (w[bnp + "/moving_mean"] * s).astype(np.float32)
    out[bnp + "/gamma"] = (w[bnp + "/gamma"] / s).astype(np.float32)
    return out


def rescaled_activation(w, block, k):
    """The tensor between conv_1 and conv_2 of residual block `block` times 2^-k: gamma and beta of batch_norm_1 times 2^-k (the
    ReLU commutes with a positive factor), the conv_2 kernel times 2^k, its bias -- which initialises the accumulator -- left
    alone.  That tensor is not on the skip path, so the network function is unchanged in exact arithmetic; every factor is a power
    of two, so it is unchanged in float32 and in every bf16 plane as long as nothing leaves the normal range."""
    out = {n: a.copy() for n, a in w.items()}
    s = np.float32(2.0) ** k
    for n in ("gamma", "beta"):
        out[f"resTower/block_{block}/batch_norm_1/{n}"] = (w[f"resTower/block_{block}/batch_norm_1/{n}"] / s).astype(np.float32)
    out[f"resTower/block_{block}/conv_2/kernel"] = (w[f"resTower/block_{block}/conv_2/kernel"] * s).astype(np.float32)
    return out


# ---- a numpy model of the split product ---------------------------------------------------------------------------------------
# (weight plane, activation plane), 0-based: the six products net_x3.hip.h and gnet_x3.hip.h keep of the nine
KERNEL_PRODUCTS = ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 0))


def split_conv(products):
    """A convolution whose operands are each rounded to float32 and split into three bf16 planes, and of whose nine plane
    products those in `products` are summed in float64 (a bf16 x bf16 product is exact in float32, let alone float64)."""
    def conv(t, k, b):
        xs = _widen(split3(t.astype(F32))).astype(np.float64)
        ws = _widen(split3(k)).astype(np.float64)
        kh = k.shape[0] // 2
        out = np.zeros(t.shape[:3] + (k.shape[3],))
        for qx in range(3):
            wsum = sum((ws[qw] for qw in range(3) if (qw, qx) in products), np.zeros(k.shape))  # products are linear in the weight planes
            tp = np.pad(xs[qx], ((0, 0), (kh, kh), (kh, kh), (0, 0)))
            for dy in range(k.shape[0]):
                for dx in range(k.shape[1]):
                    if wsum[dy, dx].any():
                        out += np.einsum("nhwc,cf->nhwf", tp[:, dy:dy + t.shape[1], dx:dx + t.shape[2], :], wsum[dy, dx])
        return out + b.astype(np.float64)
    return conv


def forward_split(w, planes, products=KERNEL_PRODUCTS, intermediates=False):
    """the statement with the tower layers' products replaced by the chosen plane products: KERNEL_PRODUCTS is the kernel model"""
    return _forward64(w, planes, intermediates=intermediates, tower_conv=split_conv(frozenset(products)))


def mutants():
    """{name: products}: the kernel model less one product, and less one plane of one operand"""
    out = {f"no w{qw + 1}.x{qx + 1}": tuple(p for p in KERNEL_PRODUCTS if p != (qw, qx)) for qw, qx in KERNEL_PRODUCTS}
    for q in range(3):
        out[f"no plane {q + 1} of the weights"] = tuple(p for p in KERNEL_PRODUCTS if p[0] != q)
        out[f"no plane {q + 1} of the activations"] = tuple(p for p in KERNEL_PRODUCTS if p[1] != q)
    return out


# ---- the contribution cases ---------------------------------------------------------------------------------------------------
A_IN = 1 + 2.0 ** -9 + 2.0 ** -18    # the activation: one bit in each bf16 plane
WV = 1 + 2.0 ** -10 + 2.0 ** -20     # the weight: one bit in each bf16 plane
GPU_TOL = 1e-6                       # the 16-filter test's tolerance against the float64 statement
SEPARATION = 100                     # every mutant moves an output by at least SEPARATION x GPU_TOL ...
HEADROOM = 1.1                       # ... the smallest of them, the lost w3.x1, by HEADROOM times that
# gamma / sqrt(moving_variance + 1e-3) of these two float32 numbers is 1 within 6e-14 in float64 and exactly 1 in float32.
# (moving_variance = 1 - 1e-3 as a float32 is 0.99900001287: the float64 statement then scales every layer by 1 - 6.4e-9 where
# the float32 forms scale by exactly 1, and behind the heads' gain below five such layers would cost 3e-6.)
BN_ID_GAMMA, BN_ID_VARIANCE = F32(1.0452781915664673), F32(1.0916064977645874)
CHANNELS = lambda F: (0, 3, 4, 7, 8, 11, 12, 15, 16, F - 1)  # both halves of a K = 32 slice, all four lane groups of tap 8, three blocks
FILTERS = lambda F: (0, 15, 16, F - 1)
CONTRIBUTION_SHAPES = [(C4, 48, 2), (TTT, 48, 2), (C4, 80, 1)]  # the wave holds 3 of 4 filter blocks; a second group with one live block


def _contribution_cases():
    cases = []
    for game, F, R in CONTRIBUTION_SHAPES:
        i = 0
        for layer in sorted({1, 2, 2 * R}):  # conv_1: no skip, planes out; conv_2: skip, planes out (R = 2); the last layer: float32 out
            for tap in range(9):
                cases.append((game, F, R, layer, tap, CHANNELS(F)[i % 10], FILTERS(F)[i % 4]))
                i += 1
    return cases


CONTRIBUTION_CASES = _contribution_cases()


def contribution_id(case):
    game, F, R, layer, tap, c, f = case
    return f"{GAME_IDS[game]}-F{F}-R{R}-l{layer}-tap{tap}-c{c}-f{f}"


def empty_board(game):
    """packed state and planes of the empty board with player 1 to move: the player plane (2) is +1 everywhere"""
    H, Wd, _ = _lib.GRID[game]
    st = _lib.pack_grid(game, np.zeros((1, H, Wd, 2), dtype=np.int8), np.ones(1, dtype=np.int64))
    gi = _lib.game_info(game)
    planes = np.zeros((1, gi.H, gi.W, gi.C), dtype=np.int8)
    planes[..., 2] = 1
    return st, planes


@functools.lru_cache(maxsize=None)
def contribution_network(case):
    """The weights of one contribution case (made once, never changed) and what the heads were set from.

    Tower: zero kernels, zero biases, identity batch norm; the first convolution puts A_IN on channel c through the centre tap
    of the player plane; tower layers before `layer` pass c on through their centre tap, `layer` holds WV at (tap, c, f), later
    layers pass f on.  The tower's output on filter f is then T0 on the cells whose `tap` neighbour is on the board and smaller
    on the others -- in the six-product model exactly a float32 (every sum stays within 24 bits), so the GPU's float32 value is
    the model's.

    Heads: the smallest defect, a lost w3.x1, takes a fraction r ~ 2^-20 off T0; the tolerance is 1e-6.  Both heads read filter f
    through ReLU(T - theta) with theta = (1 - delta) T0, delta = r / (SEPARATION x HEADROOM x GPU_TOL): the lost product moves
    every logit of weight +-1 by 1.1e-4 of itself.  The three products that the form drops by design (2^-28 + 2^-29 + 2^-38
    against w3.x1 = 2^-20: 1 / 170.6 of it) are amplified alike: the kernel model is 6.4e-7 from the statement, which is the
    closest to `far inside 1e-6` that a separation of 100 for w3.x1 leaves.  So that the GPU adds no noise of its own on top, theta
    is a multiple of 2^-17 and the dense weights are powers of two times k / 4: every product and partial sum of the policy head
    is exact in float32 in any order.  Logits lie in [1, 2), the value is tanh of half of that."""
    game, F, R, layer, tap, c, f = case
    gi = _lib.game_info(game)
    w = W.init_weights(gi.C, F, R, 16, gi.A, seed=11)
    for n, a in w.items():
        a[:] = {"gamma": BN_ID_GAMMA, "moving_variance": BN_ID_VARIANCE}.get(n.rsplit("/", 1)[1], 0)
    w["resTower/conv_block/conv/kernel"][1, 1, 2, c] = A_IN
    for l in range(1, 2 * R + 1):
        k = w[_layer_names(R)[l][0] + "/kernel"]
        if l == layer:
            k[tap // 3, tap % 3, c, f] = WV
        else:
            ch = c if l < layer else f
            k[1, 1, ch, ch] = 1
    _st, planes = empty_board(game)
    tower = lambda products: forward_split(w, planes, products, intermediates=True)[2][-1][0, :, :, f]
    T, T_lost = tower(KERNEL_PRODUCTS), tower(mutants()["no w3.x1"])
    T0 = T.max()
    # the model's tower output is a float32 with no bit below 2^-20 (up to the 6e-14 per layer of the float64 batch norm)
    assert np.abs(T * 2.0 ** 20 - np.round(T * 2.0 ** 20)).max() < 1e-6 and T0 < 8
    r = (T0 - T_lost.max()) / T0
    assert 2.0 ** -22 < r < 2.0 ** -19, r
    delta = r / (SEPARATION * HEADROOM * GPU_TOL)
    theta = np.round(T0 * (1 - delta) * 2.0 ** 17) / 2.0 ** 17
    n_in = int((T > theta).sum())
    assert n_in >= 4 and np.ptp(T[T > theta]) < 1e-12 and T[T <= theta].max(initial=0) < theta - 0.5
    gain = 2.0 ** np.ceil(np.log2(1 / (n_in * (T0 - theta))))  # the logits of weight 1 land in [1, 2)
    w["policy/convolution/kernel"][0, 0, f, 0] = 1
    w["policy/convolution/bias"][0] = -theta
    w["policy/policy/kernel"][0] = [gain * (a % 4 + 1) / 4 * (-1) ** a for a in range(gi.A)]
    w["value/convolution/kernel"][0, 0, f, 0] = 1
    w["value/convolution/bias"][0] = -theta
    w["value/dense_1/kernel"][0, 0] = gain / 2
    w["value/dense_2/kernel"][0, 0] = 1
    assert float(w["value/convolution/bias"][0]) == -theta
    return w, dict(T0=T0, theta=theta, delta=delta, r=r, n_in=n_in, gain=gain)


# ---- the envelope cases -------------------------------------------------------------------------------------------------------
ENVELOPE_SHAPES = [(C4, 48, 2), (DC, 32, 2)]  # (game, F, R); DragonChess: padded input planes, tiles that straddle rows
FUSED_SHAPE = (C4, 16, 4)                      # the 16-filter form of test_fused_split_activation_rescaling
# The first init_weights seed from 21 up with which, for EVERY case of the shape, the oracle's value and logits both move with
# the position (tests/test_split_cases_cpu.py asserts it and that no earlier seed does).  The large-activation case is held to
# the logits alone: its value head sees activations 1e4 times the usual and its tanh is saturated with every seed.
ENVELOPE_SEEDS = {(C4, 48): 21, (DC, 32): 24, (C4, 16): 40}


def live(v, l):
    """both heads see the position: the rule of tests/test_gpu_gnet_batch.py"""
    return bool(np.ptp(v) >= 0.05 and np.abs(v).max() < 0.999 and np.ptp(l, axis=0).max() >= 0.3)


def case_is_live(kind, v, l):
    return live(v, l) if kind != "two-sided" else bool(np.ptp(l, axis=0).max() >= 0.3)


@functools.lru_cache(maxsize=None)
def envelope_positions(game, F):
    """(packed states, the indices the oracle and the float64 statement see).  Wide shapes: the smallest ragged batch that ROWS of
    tests/test_gpu_gnet_batch.py lists for (game, F) and its _oracle_subset; the 16-filter form: 24 boards, all of them."""
    from tests.net_cases import positions
    if F == 16:
        return positions(game, 24, seed=3), np.arange(24)
    from tests.test_gpu_gnet_batch import ROWS, _oracle_subset
    n = next(ns[game] for f, _r, ns in ROWS if f == F)
    return positions(game, n, seed=F + n), _oracle_subset(game, n)


def envelope_weights(game, F, R, seed=None):
    gi = _lib.game_info(game)
    return W.init_weights(gi.C, F, R, 16, gi.A, seed=ENVELOPE_SEEDS[game, F] if seed is None else seed, perturb=True)


def large_activations(w):
    """tiny variances and large gammas on the first two layers: activations beyond 1e4"""
    big = {n: a.copy() for n, a in w.items()}
    big["resTower/conv_block/batch_norm/moving_variance"][:] = 1e-8
    big["resTower/conv_block/batch_norm/gamma"] *= 64.0
    big["resTower/block_0/batch_norm_1/moving_variance"][:] = 1e-8
    big["resTower/block_0/batch_norm_1/gamma"] *= 64.0
    return big


def envelope_cases(w, R, wide=True):
    """[(name, weights, kind)]: kind "base"; "bits": the same function in powers of two, the base's bits; "two-sided": checked
    against the oracle and the float64 statement; "subnormal": so too, in the corner where a third plane is a bf16 subnormal.
    wide = False: only the activation rescalings (what the 16-filter form's own envelope test leaves out)."""
    cases = [("base", w, "base")]
    if wide:
        for layer in (0, 1, 2, 2 * R):
            for k in (20, -20, 12, -12):
                cases.append((f"layer {layer} x 2^{k}", _rescaled(w, layer, k, R), "bits"))
    for block in (0, R - 1):
        for k in (20, -20):
            cases.append((f"block {block} activation x 2^{-k}", rescaled_activation(w, block, k), "bits"))
    if wide:
        cases.append(("variance 1e-8, gamma x 64", large_activations(w), "two-sided"))
        cases.append(("layer 1 x 2^-112 (third weight plane subnormal)", _rescaled(w, 1, -112, R), "subnormal"))
    cases.append(("block 0 activation x 2^-112 (third activation plane subnormal)", rescaled_activation(w, 0, 112), "subnormal"))
    return cases


def oracle_planes(orc, game, st):
    """the input planes of packed states by the oracle's encoder: what _lib.game_encode gives, without a GPU"""
    from tests.selfplay_cases import OG, orc_state_from_packed
    return np.concatenate([orc.encode(OG[game], orc_state_from_packed(orc, OG[game], game, s)) for s in st])
