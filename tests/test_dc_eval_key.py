"""The DragonChess evaluation cache's position key (games.hip.h DragonChess::cache_key, DCKey) is exact: on every position up
to ply 6 from the start, on the positions of random games and on hand-built pairs that differ in one castle flag or only in
plane 16, equal keys mean equal network inputs (encode_cell's 17 planes), and no key is all-zero.  States the network never
sees in play (a piece code outside -6 .. 6, a castle flag other than 0 / 1) get no key.  The header is compiled for the host
with hipcc; no GPU is needed."""
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
#include <cstring>
#include <random>
#include <string>
#include <unordered_map>
#include <vector>
using G = DragonChess;
struct KeyHash { size_t operator()(const DCKey &k) const { return (size_t)k.tag(); } };
// the network input of a position, as encode_cell forms it: the 17 planes of every cell
static std::string input_of(const G::State &s) {
    std::string in(64 * 17, '\0');
    for (int r = 0; r < 8; r++)
        for (int c = 0; c < 8; c++) {
            int8_t v[17];
            G::encode_cell(s, r, c, v);
            memcpy(&in[(r * 8 + c) * 17], v, 17);
        }
    return in;
}
static std::unordered_map<DCKey, std::string, KeyHash> seen;
static long n_checked = 0, n_bad = 0;
static DCKey check(const G::State &s) {
    const DCKey k = G::cache_key(s);
    n_checked++;
    if (k.none()) { n_bad++; return k; }
    const std::string in = input_of(s);
    auto it = seen.find(k);
    if (it == seen.end()) seen.emplace(k, in);
    else if (it->second != in) n_bad++;
    return k;
}
static std::vector<int> moves(const G::State &s) {
    std::vector<int> m;
    for (int sq1 = 0; sq1 < 64; sq1++) {
        const int p = s.b[sq1];
        if (!p || (p > 0) != (s.player == 1)) continue;
        for (uint64_t t = G::targets(s, sq1); t; t &= t - 1) m.push_back(G::action_id(sq1, bb_ctz64(t)));
    }
    return m;
}
static void walk(const G::State &s, int ply, int depth) {
    check(s);
    if (ply == depth) return;
    for (int a : moves(s)) {
        G::State t = s;
        if (!G::apply(t, a)) { n_bad++; continue; } // (targets and apply disagree: not this test's subject, but loud)
        if (G::winner(t, -1) >= 0) { check(t); continue; } // the game ends here: nothing is evaluated beyond
        walk(t, ply + 1, depth);
    }
}
int main(int argc, char **argv) {
    const int depth = atoi(argv[1]);
    const long n_games = atol(argv[2]);
    walk(G::initial(), 0, depth);
    const size_t tree = seen.size();
    std::mt19937_64 rng(12345);
    for (long i = 0; i < n_games; i++) {
        G::State s = G::initial();
        const int len = (int)(rng() % 300);
        for (int p = 0; p < len; p++) {
            const std::vector<int> m = moves(s);
            if (m.empty()) break;
            G::apply(s, m[rng() % m.size()]);
            check(s);
            if (G::winner(s, -1) >= 0) break;
        }
    }
    // pairs that differ in one input plane only: different keys
    long n_pairs = 0;
    auto differ = [&](const G::State &a, const G::State &b) {
        n_pairs++;
        if (input_of(a) == input_of(b) || check(a) == check(b)) n_bad++;
    };
    for (int f = 0; f < 4; f++) { // one castle flag
        G::State a = G::initial(), b = a;
        b.castle[f] ^= 1;
        differ(a, b);
    }
    { // plane 16 alone: White's first move of two (player 1 after Black) against its second (player 1 after player 1)
        G::State a = G::initial(), b = a;
        a.prev = 2;
        b.prev = 1;
        differ(a, b);
        G::State c = a; // Black to move after White's two moves: plane 16 is 0 as for White's first move
        c.player = 2;
        c.prev = 1;
        if (!(check(a) == check(c))) n_bad++; // (the same network input: a key does not have to, but this one does)
    }
    { // one piece code on one square, for every square and code
        const G::State a = G::initial();
        for (int sq = 0; sq < 64; sq++)
            for (int v = -6; v <= 6; v++) {
                if (v == a.b[sq]) continue;
                G::State b = a;
                b.b[sq] = (int8_t)v;
                differ(a, b);
            }
    }
    { // states the network never sees in play: no key
        G::State a = G::initial(), b = a;
        a.b[20] = 7;
        b.castle[2] = 2;
        if (!G::cache_key(a).none() || !G::cache_key(b).none()) n_bad++;
    }
    printf("checked %ld positions, %zu distinct keys (%zu up to ply %d), %ld differing pairs, bad %ld\n", n_checked,
           seen.size(), tree, depth, n_pairs, n_bad);
    return n_bad ? 1 : 0;
}
"""


def test_dc_cache_key_exact(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not found (set HIPCC)")
    src = tmp_path / "key.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "key"
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-O2", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe), "6", "1000"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    # every position up to ply 6 is walked (W, W, B, W, W, B: 1.5e5 distinct ones)
    n_tree = int(out.stdout.split("(")[1].split()[0])
    assert n_tree > 100000, out.stdout
