"""The two-way buckets of the Connect4 evaluation cache (net.hip.h): which way of its bucket a missed position is stored into
(games.hip.h eval_cache_pick_way) and the stone count that ranks two positions (GridGame::key_stones), both read off the keys.

The rule, as the store path applies it to the eight chunk keys its probe has read: an empty or torn way is taken first (way 0
before way 1); otherwise way 0 keeps the shallower position -- it is replaced only by a position with no more stones than its
occupant -- and way 1 is always replaced.  The header is compiled for the host with hipcc; no GPU is needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from blackbird_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blackbird_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

PROGRAM = r"""
#include "games.hip.h"
#include <cstdio>
#include <random>
using G = Connect4;
static long n_bad = 0;
static void expect(bool ok, const char *what) {
    if (!ok) { n_bad++; printf("FAILED: %s\n", what); }
}
// a position `moves` plies into a game that drops its stones left to right, row by row (no four in a row is looked for:
// only the key matters here)
static uint64_t key_after(int moves) {
    G::State s = G::initial();
    for (int p = 0; p < moves; p++) G::apply(s, p % G::W);
    return G::cache_key(s);
}
static int pick(uint64_t key, uint64_t a0, uint64_t a1, uint64_t a2, uint64_t a3, uint64_t b0, uint64_t b1, uint64_t b2, uint64_t b3) {
    const uint64_t k[8] = {a0, a1, a2, a3, b0, b1, b2, b3};
    return eval_cache_pick_way_of<G>(key, k);
}
int main(int argc, char **argv) {
    // ---- the way-selection rule over hand-made buckets ----
    const uint64_t TOMOVE = 1ull << 63;
    const uint64_t k2 = key_after(2), k5 = key_after(5), k5b = key_after(5) ^ 1ull /* column 0's lowest stone changes hands */,
                   k9 = key_after(9), k12 = key_after(12), k2o = k2 ^ TOMOVE;
    expect(k2 && k5 && k9 && k12, "keys");
    expect(G::key_stones(k2) == 2 && G::key_stones(k5) == 5 && G::key_stones(k5b) == 5 && G::key_stones(k9) == 9 &&
               G::key_stones(k12) == 12 && G::key_stones(k2o) == 2 && G::key_stones(G::cache_key(G::initial())) == 0,
           "stones of the hand-made keys");
    expect(pick(k5, 0, 0, 0, 0, 0, 0, 0, 0) == 0, "empty bucket: way 0");
    expect(pick(k5, 0, 0, 0, 0, k2, k2, k2, k2) == 0, "way 0 empty, way 1 full: way 0");
    expect(pick(k5, k2, k2, k2, k2, 0, 0, 0, 0) == 1, "way 0 full, way 1 empty: way 1");
    expect(pick(k2, k9, k9, k9, k9, 0, 0, 0, 0) == 1, "way 1 empty: taken before the kept way is fought over");
    expect(pick(k5, k2, k2, k9, k2, k12, k12, k12, k12) == 0, "way 0 torn (two keys): free");
    expect(pick(k5, k2, k2, k2, 0, k12, k12, k12, k12) == 0, "way 0 torn (a chunk still empty): free");
    expect(pick(k5, k2, k2, k2, k2, k12, k9, k12, k12) == 1, "way 1 torn: free");
    expect(pick(k5, k2, k2, k2, k2, k12, k12, k12, k12) == 1, "shallower occupant in way 0: kept, way 1 replaced");
    expect(pick(k5, k2, k2, k2, k2, k2o, k2o, k2o, k2o) == 1, "way 1 is replaced whatever it holds");
    expect(pick(k5, k9, k9, k9, k9, k12, k12, k12, k12) == 0, "deeper occupant in way 0: replaced");
    expect(pick(k5, k9, k9, k9, k9, k2, k2, k2, k2) == 0, "deeper occupant in way 0: replaced, whatever way 1 holds");
    expect(pick(k5, k5b, k5b, k5b, k5b, k12, k12, k12, k12) == 0, "equal stones: way 0 is replaced (no more stones than its occupant)");
    expect(pick(k5 ^ TOMOVE, k5, k5, k5, k5, k12, k12, k12, k12) == 0, "the player bit is no stone");
    // ---- the stone count from keys: the boards of the fixture file (p1 p2 stones per line) ... ----
    long n_keyed = 0, n_lines = 0;
    FILE *f = fopen(argv[1], "r");
    unsigned long long p1, p2;
    int stones;
    while (f && fscanf(f, "%llu %llu %d", &p1, &p2, &stones) == 3) {
        G::State s;
        s.p1 = p1;
        s.p2 = p2;
        n_lines++;
        const uint64_t k = G::cache_key(s);
        if (!k) continue; // not one stack of stones per column: no key
        n_keyed++;
        if (G::key_stones(k) != stones) n_bad++;
    }
    // ---- ... and 10^5 positions of random play ----
    std::mt19937_64 rng(4321);
    long n_random = 0;
    for (int i = 0; i < 100000; i++) {
        G::State s = G::initial();
        const int len = (int)(rng() % (G::H * G::W + 1));
        for (int p = 0; p < len; p++) {
            const uint32_t m = G::legal_mask(s);
            if (!m) break;
            int a;
            do a = (int)(rng() % G::A); while (!((m >> a) & 1));
            G::apply(s, a);
        }
        const uint64_t k = G::cache_key(s);
        n_random++;
        if (!k || G::key_stones(k) != bb_popc64(gs_cells(s.p1) | gs_cells(s.p2))) n_bad++;
    }
    printf("fixture boards %ld keyed %ld random %ld bad %ld\n", n_lines, n_keyed, n_random, n_bad);
    return n_bad ? 1 : 0;
}
"""


def test_pick_way_and_key_stones(tmp_path, golden_dir):
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not found (set HIPCC)")
    g = np.load(os.path.join(golden_dir, "boards_c4.npz"))
    H, W, _ = _lib.GRID[_lib.GAME_CONNECT4]
    boards = g["board"].reshape(-1, H, W, 2)
    packed = _lib.pack_grid(_lib.GAME_CONNECT4, boards, g["player"], g["prev"])
    # popcount of the boards (a board on which both planes claim one cell has no key and is not compared)
    stones = (boards != 0).any(axis=3).reshape(len(boards), -1).sum(axis=1)
    lines = tmp_path / "boards.txt"
    lines.write_text("".join("%d %d %d\n" % (int(p[0]), int(p[1]), int(s)) for p, s in zip(packed, stones)))
    src = tmp_path / "ways.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "ways"
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-O2", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe), str(lines)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    w = out.stdout.split()
    assert int(w[2]) == len(boards) and int(w[4]) > 0, out.stdout   # every fixture board was read, some of them carry a key
