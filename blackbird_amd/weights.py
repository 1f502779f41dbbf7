"""Weight container for the residual tower + heads.

Variables carry the names the reference's TensorFlow graph gives them
(/root/reference/src/NetworkFactory.py:22-183, scopes `resTower/conv_block`, `resTower/block_{i}`,
`value`, `policy`), so a checkpoint exported from the original as name->array can be loaded as is
(SURVEY.md 2.3 / 8f-f4).  `flatten()` regroups them into the contiguous float32 blocks the C ABI
(include/blackbird_hip.h: bb_net_weights) takes.
"""
import re

import numpy as np

BN_FIELDS = ("gamma", "beta", "moving_mean", "moving_variance")


def variable_names(blocks):
    names = ["resTower/conv_block/conv/kernel", "resTower/conv_block/conv/bias"]
    names += [f"resTower/conv_block/batch_norm/{f}" for f in BN_FIELDS]
    for i in range(blocks):
        for j in (1, 2):
            names += [f"resTower/block_{i}/conv_{j}/kernel", f"resTower/block_{i}/conv_{j}/bias"]
            names += [f"resTower/block_{i}/batch_norm_{j}/{f}" for f in BN_FIELDS]
    for head in ("value", "policy"):
        names += [f"{head}/convolution/kernel", f"{head}/convolution/bias"]
        names += [f"{head}/batch_norm/{f}" for f in BN_FIELDS]
    names += ["value/dense_1/kernel", "value/dense_1/bias", "value/dense_2/kernel", "value/dense_2/bias",
              "policy/policy/kernel", "policy/policy/bias"]
    return names


def _glorot(rng, shape):
    # TF default kernel_initializer = glorot_uniform: limit = sqrt(6 / (fan_in + fan_out)),
    # fan_in = prod(shape[:-2]) * shape[-2], fan_out = prod(shape[:-2]) * shape[-1]
    rf = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
    fan_in, fan_out = rf * shape[-2], rf * shape[-1]
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, size=shape).astype(np.float32)


def init_weights(in_planes, filters, blocks, dense, actions, seed=0, perturb=False):
    """Random-init weights as `global_variables_initializer` would leave them (Network.py:23):
    glorot-uniform kernels, zero biases, gamma=1, beta=0, moving_mean=0, moving_variance=1.
    perturb=True also randomises biases and batch-norm statistics (used by parity tests so that
    every term of the graph is exercised)."""
    rng = np.random.RandomState(seed)
    C, F, D, A = in_planes, filters, dense, actions
    w = {}

    def bn(prefix, n):
        if perturb:
            w[f"{prefix}/gamma"] = rng.uniform(0.5, 1.5, n).astype(np.float32)
            w[f"{prefix}/beta"] = rng.uniform(-0.3, 0.3, n).astype(np.float32)
            w[f"{prefix}/moving_mean"] = rng.uniform(-0.3, 0.3, n).astype(np.float32)
            w[f"{prefix}/moving_variance"] = rng.uniform(0.5, 2.0, n).astype(np.float32)
        else:
            w[f"{prefix}/gamma"] = np.ones(n, np.float32)
            w[f"{prefix}/beta"] = np.zeros(n, np.float32)
            w[f"{prefix}/moving_mean"] = np.zeros(n, np.float32)
            w[f"{prefix}/moving_variance"] = np.ones(n, np.float32)

    def bias(name, n):
        w[name] = (rng.uniform(-0.2, 0.2, n) if perturb else np.zeros(n)).astype(np.float32)

    w["resTower/conv_block/conv/kernel"] = _glorot(rng, (3, 3, C, F))
    bias("resTower/conv_block/conv/bias", F)
    bn("resTower/conv_block/batch_norm", F)
    for i in range(blocks):
        for j in (1, 2):
            w[f"resTower/block_{i}/conv_{j}/kernel"] = _glorot(rng, (3, 3, F, F))
            bias(f"resTower/block_{i}/conv_{j}/bias", F)
            bn(f"resTower/block_{i}/batch_norm_{j}", F)
    w["value/convolution/kernel"] = _glorot(rng, (1, 1, F, 1))
    bias("value/convolution/bias", 1)
    bn("value/batch_norm", 1)
    w["value/dense_1/kernel"] = _glorot(rng, (1, D))
    bias("value/dense_1/bias", D)
    w["value/dense_2/kernel"] = _glorot(rng, (D, 1))
    bias("value/dense_2/bias", 1)
    w["policy/convolution/kernel"] = _glorot(rng, (1, 1, F, 2))
    bias("policy/convolution/bias", 2)
    bn("policy/batch_norm", 2)
    w["policy/policy/kernel"] = _glorot(rng, (2, A))
    bias("policy/policy/bias", A)
    return w


def infer_shape(w):
    k0 = w["resTower/conv_block/conv/kernel"]
    C, F = k0.shape[2], k0.shape[3]
    R = 0
    while f"resTower/block_{R}/conv_1/kernel" in w:
        R += 1
    D = w["value/dense_1/kernel"].shape[1]
    A = w["policy/policy/kernel"].shape[1]
    return C, F, R, D, A


# One row per float block of bb_net_weights, in the struct's order: the field, the block's shape in the letters of
# infer_shape(), the TF variables it is made of back to back -- `{i}`, `{j}`: one per residual block i and convolution j = 1, 2
# of it; `/*`: the four BN_FIELDS, in their order -- and the TF shape of one of those variables where it is not the block's own
# shape behind the dimensions the expansions account for ([R][2] and [4]).
BLOCKS = (
    ("conv0_k", (3, 3, "C", "F"), "resTower/conv_block/conv/kernel", None),
    ("conv0_b", ("F",), "resTower/conv_block/conv/bias", None),
    ("conv0_bn", (4, "F"), "resTower/conv_block/batch_norm/*", None),
    ("blk_k", ("R", 2, 3, 3, "F", "F"), "resTower/block_{i}/conv_{j}/kernel", None),
    ("blk_b", ("R", 2, "F"), "resTower/block_{i}/conv_{j}/bias", None),
    ("blk_bn", ("R", 2, 4, "F"), "resTower/block_{i}/batch_norm_{j}/*", None),
    ("v_conv_k", ("F",), "value/convolution/kernel", (1, 1, "F", 1)),
    ("v_conv_b", (1,), "value/convolution/bias", None),
    ("v_bn", (4, 1), "value/batch_norm/*", None),
    ("v_d1_k", ("D",), "value/dense_1/kernel", (1, "D")),
    ("v_d1_b", ("D",), "value/dense_1/bias", None),
    ("v_d2_k", ("D",), "value/dense_2/kernel", ("D", 1)),
    ("v_d2_b", (1,), "value/dense_2/bias", None),
    ("p_conv_k", ("F", 2), "policy/convolution/kernel", (1, 1, "F", 2)),
    ("p_conv_b", (2,), "policy/convolution/bias", None),
    ("p_bn", (4, 2), "policy/batch_norm/*", None),
    ("p_d_k", (2, "A"), "policy/policy/kernel", None),
    ("p_d_b", ("A",), "policy/policy/bias", None),
)
FIELDS = tuple(row[0] for row in BLOCKS)


def blocks(C, F, R, D, A):
    """BLOCKS at one shape: [(field, the block's shape, its TF variables in order, the TF shape of one of them)]."""
    dims = dict(C=C, F=F, R=R, D=D, A=A)
    rows = []
    for field, shape, pattern, var_shape in BLOCKS:
        shape = tuple(dims.get(n, n) for n in shape)
        per_block, bn = "{i}" in pattern, pattern.endswith("/*")
        names = [pattern.format(i=i, j=j) for i in range(R) for j in (1, 2)] if per_block else [pattern]
        if bn:
            names = [n[:-1] + f for n in names for f in BN_FIELDS]
        var_shape = tuple(dims.get(n, n) for n in var_shape) if var_shape else shape[2 * per_block + bn:]
        rows.append((field, shape, names, var_shape))
    return rows


def flatten(w):
    """TF-named dict -> dict of contiguous float32 blocks named like bb_net_weights' fields."""
    out = {}
    for field, shape, names, _ in blocks(*infer_shape(w)):
        parts = [np.ascontiguousarray(w[n], dtype=np.float32) for n in names]
        if len(parts) != 1:   # (one variable: the block is that variable, reshaped)
            parts = [np.concatenate([np.zeros(0, np.float32)] + [p.ravel() for p in parts])]
        out[field] = parts[0].reshape(shape)
    return out


def flat_fields(C, F, R, D, A):
    """(bb_net_weights field, shape) in the struct's order: how bb_trainer_read lays one flat vector out."""
    return [(field, shape) for field, shape, _, _ in blocks(C, F, R, D, A)]


def unflatten(vec, C, F, R, D, A):
    """The inverse of flatten() for one flat float32 vector in flat_fields' order: the TF-named dict, fresh arrays."""
    vec = np.asarray(vec)
    w, at = {}, 0
    for _, _, names, var_shape in blocks(C, F, R, D, A):
        n = int(np.prod(var_shape))
        for name in names:
            w[name] = vec[at:at + n].reshape(var_shape).copy()
            at += n
    assert at == vec.size, (at, vec.size)
    # in init_weights' order: a residual block's variables stand together, where the struct has all kernels, then all biases ...
    block_of = lambda name: [int(x) for x in re.findall(r"_(\d+)/", name)] if "/block_" in name else None  # noqa: E731
    tower = iter(sorted((name for name in w if block_of(name)), key=block_of))   # (stable: kernel, bias, batch norm of each i, j)
    return {name: w[name] for name in (next(tower) if block_of(name) else name for name in w)}


def save_npz(path, w):
    np.savez(path, **{k.replace("/", "."): v for k, v in w.items()})


def load_npz(path):
    with np.load(path, allow_pickle=False) as z:
        return {k.replace(".", "/"): z[k] for k in z.files}
