"""The evaluation cache's position key (games.hip.h GridGame::cache_key) is exact: on every Connect4 position up to ply 8 and on
10^6 random positions reached in play, equal keys mean equal network inputs (encode_cell's three planes), and no key is 0.
The header is compiled for the host with hipcc; no GPU is needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blackbird_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

PROGRAM = r"""
#include "games.hip.h"
#include <cstdio>
#include <random>
#include <unordered_map>
#include <utility>
using G = Connect4;
// the network input of a position, as encode_cell forms it: (plane 0, plane 1) over the board cells, plane 2's sign
struct Input { uint64_t a, b; int me; bool operator==(const Input &o) const { return a == o.a && b == o.b && me == o.me; } };
static Input input_of(const G::State &s) {
    Input in{0, 0, 0};
    for (int r = 0; r < G::H; r++)
        for (int c = 0; c < G::W; c++) {
            int8_t v[3];
            G::encode_cell(s, r, c, v);
            in.a |= (uint64_t)v[0] << (r * G::W + c);
            in.b |= (uint64_t)v[1] << (r * G::W + c);
            in.me = v[2];
        }
    return in;
}
static std::unordered_map<uint64_t, Input> seen;
static long n_checked = 0, n_bad = 0;
static void check(const G::State &s) {
    const uint64_t k = G::cache_key(s);
    n_checked++;
    if (k == 0) { n_bad++; return; }
    const Input in = input_of(s);
    auto it = seen.find(k);
    if (it == seen.end()) seen.emplace(k, in);
    else if (!(it->second == in)) n_bad++;
}
static void walk(const G::State &s, int ply, int depth) {
    check(s);
    if (ply == depth) return;
    for (int a = 0; a < G::A; a++) {
        G::State t = s;
        if (!G::apply(t, a)) continue;
        if (G::winner(t, a) >= 0) { check(t); continue; } // the game ends here: nothing is evaluated beyond
        walk(t, ply + 1, depth);
    }
}
int main(int argc, char **argv) {
    const int depth = atoi(argv[1]);
    const long n_random = atol(argv[2]);
    walk(G::initial(), 0, depth);
    const size_t tree = seen.size();
    std::mt19937_64 rng(12345);
    for (long i = 0; i < n_random; i++) {
        G::State s = G::initial();
        const int len = (int)(rng() % (G::H * G::W + 1));
        for (int p = 0; p < len; p++) {
            const uint32_t m = G::legal_mask(s);
            if (!m) break;
            int a;
            do a = (int)(rng() % G::A); while (!((m >> a) & 1));
            G::apply(s, a);
            if (G::winner(s, a) >= 0) break;
        }
        check(s);
    }
    // boards that are not one stack of stones per column have no key
    G::State f = gs_make(1ull << (2 * G::STR + 3), 0, 1, 0); // a stone in mid-air
    G::State o = gs_make(1, 1, 1, 0);                         // both planes on one cell
    if (G::cache_key(f) != 0 || G::cache_key(o) != 0) n_bad++;
    printf("checked %ld positions, %zu distinct keys (%zu up to ply %d), bad %ld\n", n_checked, seen.size(), tree, depth, n_bad);
    return n_bad ? 1 : 0;
}
"""


def test_cache_key_exact(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not found (set HIPCC)")
    src = tmp_path / "key.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "key"
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-O2", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe), "8", "1000000"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    # every position up to ply 8 is walked (2.6e5 distinct ones)
    n_tree = int(out.stdout.split("(")[1].split()[0])
    assert n_tree > 100000, out.stdout
