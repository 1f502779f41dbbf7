"""BB_NET_BLOCKS (include/blackbird_hip.h), the one table of bb_net_weights' float blocks, printed by a stand-alone program through
csrc/net_blocks.h and held to the Python table (weights.flat_fields, weights.flatten) and to sizes restated here: names, counts
and offsets, how many floats the trainer takes for moving statistics (kind 0), for the L2 mean (kind 1) and for biases (kind 2),
and the number of variables in the L2 mean.  No GPU and no libblackbird_hip.so."""
import subprocess

import numpy as np
import pytest

from blackbird_amd import weights as W
from tests.host_cases import CSRC, host_compiler

PROGRAM = r"""
#include "net_blocks.h"
#include <cstdio>
#include <cstdlib>
// C F R D A -> a line `name count offset kind0 kind1 kind2` per block, then `total count n_l2`
int main(int argc, char **argv) {
    if (argc != 6) return 2;
    const NetBlocks t = net_blocks(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
    const std::vector<uint8_t> kind = net_block_kinds(t);
    if (kind.size() != (size_t)t.count) return 3;
    for (const NetBlock &b : t.b) {
        int n[3] = {0, 0, 0};
        for (int i = b.at; i < b.at + b.count(); i++) {
            if (kind[i] > 2) return 4;
            n[kind[i]]++;
        }
        printf("%s %d %d %d %d %d\n", b.name, b.count(), b.at, n[0], n[1], n[2]);
    }
    printf("total %d %d\n", t.count, net_blocks_l2(t));
    bb_net_weights w = {};
    if (!net_block_missing(w)) return 5; // (nothing given)
    return 0;
}
"""

SHAPES = [(3, 16, 0, 1, 7), (3, 16, 2, 10, 7), (3, 16, 9, 64, 9), (17, 16, 1, 10, 4032)]  # C, F, R, D, A
NAMES = ["conv0_k", "conv0_b", "conv0_bn", "blk_k", "blk_b", "blk_bn", "v_conv_k", "v_conv_b", "v_bn", "v_d1_k", "v_d1_b",
         "v_d2_k", "v_d2_b", "p_conv_k", "p_conv_b", "p_bn", "p_d_k", "p_d_b"]


def _sizes(C, F, R, D, A):
    """the sizes as tests/test_net_pack_cpu.py's make_net spells them"""
    return [9 * C * F, F, 4 * F, R * 2 * 9 * F * F, R * 2 * F, R * 2 * 4 * F, F, 1, 4, D, D, D, 1, 2 * F, 2, 8, 2 * A, A]


@pytest.fixture(scope="module")
def table_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("weight_blocks")
    src, exe = d / "blocks.cpp", d / "blocks"
    src.write_text(PROGRAM)
    subprocess.check_call([host_compiler(), "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-I", CSRC,
                           str(src), "-o", str(exe)])
    return str(exe)


@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(map(str, s)) for s in SHAPES])
def test_the_c_table_is_the_python_table(table_program, shape):
    C, F, R, D, A = shape
    lines = [ln.split() for ln in subprocess.check_output([table_program] + [str(x) for x in shape], text=True).splitlines()]
    rows, (tag, total, n_l2) = [(ln[0], [int(x) for x in ln[1:]]) for ln in lines[:-1]], lines[-1]
    assert tag == "total" and len(rows) == 18
    names, counts, offsets = [r[0] for r in rows], [r[1][0] for r in rows], [r[1][1] for r in rows]
    fields = W.flat_fields(C, F, R, D, A)
    assert names == [n for n, _s in fields] == NAMES == list(W.FIELDS)
    assert counts == [int(np.prod(s)) for _n, s in fields] == _sizes(C, F, R, D, A)
    assert offsets == [int(x) for x in np.cumsum([0] + counts[:-1])]
    flat = W.flatten(W.init_weights(C, F, R, D, A, seed=1))
    assert int(total) == sum(counts) == sum(x.size for x in flat.values())
    kinds = np.array([r[1][2:] for r in rows])
    assert (kinds.sum(axis=1) == counts).all()
    for name, n, k in zip(names, counts, kinds.tolist()):  # a kernel is all 1, a bias all 2, a batch norm half 1 and half 0
        assert k == ([n // 2, n // 2, 0] if name.endswith("_bn") else [0, 0, n] if name.endswith("_b") else [0, n, 0]), name
    assert kinds[:, 0].sum() == 2 * F * (1 + 2 * R) + 2 + 4            # moving mean and variance of every batch norm
    assert kinds[:, 2].sum() == F + 2 * R * F + 1 + D + 1 + 2 + A      # every bias
    assert int(n_l2) == 12 + 6 * R
