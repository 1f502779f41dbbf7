"""Stand-alone host programs of the CPU tests (not collected; needs no library): the compiler they are built with, and the
board symmetries as csrc/symmetry.h computes them -- a program compiled from the header alone prints them, the `maps` fixture
parses what it prints."""
import os
import shutil
import subprocess

import numpy as np
import pytest


def host_compiler():
    for c in (os.environ.get("CXX"), "g++", "clang++", "c++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if c and (shutil.which(c) or os.path.exists(c)):
            return c
    pytest.fail("no host C++ compiler found (set CXX)")


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blackbird_amd", "csrc")
C4, TTT, DC = 0, 1, 2  # BB_GAME_*
SHAPE = {C4: (6, 7, 7), TTT: (3, 3, 9), DC: (8, 8, 4032)}  # H, W, A
NSYM = {C4: 2, TTT: 8, DC: 1}

PROGRAM = r"""
#include "symmetry.h"
#include <cstdio>
template <int GAME>
static void show() {
    using S = Symmetries<GAME>;
    static_assert(S::cell(0, 0) == 0 && S::inverse(0) == 0, "usable in constant expressions");
    printf("game %d %d %d %d %d %d\n", GAME, S::NSYM, S::H, S::W, S::A, game_symmetries(GAME));
    for (int s = 0; s < S::NSYM; s++) {
        printf("inverse %d %d\n", s, S::inverse(s));
        printf("cell %d", s);
        for (int i = 0; i < S::H * S::W; i++) printf(" %d", S::cell(s, i));
        printf("\ncell_inv %d", s);
        for (int i = 0; i < S::H * S::W; i++) printf(" %d", S::cell_inv(s, i));
        printf("\naction %d", s);
        for (int a = 0; a < S::A; a++) printf(" %d", S::action(s, a));
        printf("\naction_inv %d", s);
        for (int a = 0; a < S::A; a++) printf(" %d", S::action_inv(s, a));
        printf("\n");
    }
}
int main() {
    show<0>();
    show<1>();
    show<2>();
    printf("unknown %d %d\n", game_symmetries(3), game_symmetries(-1));
    return 0;
}
"""


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    """{game: dict(nsym, inverse [nsym], cell, cell_inv [nsym][H*W], action, action_inv [nsym][A])} as the header computes them"""
    d = tmp_path_factory.mktemp("symmetry")
    src = d / "sym.cpp"
    src.write_text(PROGRAM)
    exe = d / "sym"
    subprocess.check_call([host_compiler(), "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True)
    res, game = {}, None
    for line in out.splitlines():
        w = line.split()
        if w[0] == "game":
            game = int(w[1])
            assert (int(w[3]), int(w[4]), int(w[5])) == SHAPE[game] and w[2] == w[6]
            res[game] = dict(nsym=int(w[2]), inverse={}, cell={}, cell_inv={}, action={}, action_inv={})
        elif w[0] == "unknown":
            assert w[1:] == ["-1", "-1"]
        elif w[0] == "inverse":
            res[game]["inverse"][int(w[1])] = int(w[2])
        else:
            res[game][w[0]][int(w[1])] = np.array(w[2:], dtype=np.int64)
    for g in res.values():
        for k in ("inverse", "cell", "cell_inv", "action", "action_inv"):
            assert sorted(g[k]) == list(range(g["nsym"])), k
            g[k] = np.array([g[k][s] for s in range(g["nsym"])])
    return res
