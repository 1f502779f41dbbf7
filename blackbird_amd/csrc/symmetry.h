// symmetry.h -- the board symmetries of the games, for training batches in another orientation (bb_examples_to_batch_sym:
// examples.hip.h).  Plain C++17 and nothing of HIP, constexpr throughout: the kernels call the same functions a stand-alone
// program prints on the host (tests/test_symmetry_cpu.py, which also holds them against the rules of the games).
//
// Symmetries<GAME>, GAME = BB_GAME_*, gives
//     NSYM                     the number of symmetries; index 0 is the identity
//     cell(s, i)               where cell i = r * W + c goes: r' * W + c'
//     action(s, a)             where action a goes, as the rules imply: the transformed position after action(s, a) is the
//                              transform of the position after a
//     inverse(s)               the index of the inverse symmetry
//     cell_inv(s, i), action_inv(s, a)   the inverse maps (what a gathering kernel asks: which cell, which action lands here?)
// s must be < NSYM: the callers check it before they come here.  No tables and no switch: a map is a few selects.
//
// Connect4 (6 x 7, an action is a column), NSYM = 2:
//     0  identity
//     1  column mirror: (r, c) -> (r, W-1-c), a -> W-1-a                       np.flip(b, axis=1)
// TicTacToe (3 x 3, an action is the cell r * W + c and goes with its cell), NSYM = 8, the dihedral group of the square.
// s = T + 2 R + 4 C: transpose first when T, then reverse the rows when R, then reverse the columns when C.  As images of a
// board b[r][c]:
//     0  identity                    b
//     1  transpose                   b.T                  (r, c) -> (c, r)
//     2  rows reversed               np.flipud(b)         (r, c) -> (N-1-r, c)
//     3  quarter turn, anticlockwise np.rot90(b, 1)       (r, c) -> (N-1-c, r)
//     4  columns reversed            np.fliplr(b)         (r, c) -> (r, N-1-c)
//     5  quarter turn, clockwise     np.rot90(b, -1)      (r, c) -> (c, N-1-r)
//     6  half turn                   np.rot90(b, 2)       (r, c) -> (N-1-r, N-1-c)
//     7  anti-transpose              np.rot90(b, 2).T     (r, c) -> (N-1-c, N-1-r)
//     Every one is its own inverse but the quarter turns, which are each other's.
// DragonChess, NSYM = 1: its start position is not mirror-symmetric (White is a king and three pawns, Black a full army), pawns
// move one way and White moves twice -- no reflection or rotation of the board maps the rules onto themselves.
#pragma once

template <int GAME>
struct Symmetries;

template <> // BB_GAME_CONNECT4
struct Symmetries<0> {
    static constexpr int H = 6, W = 7, A = 7, NSYM = 2;
    static constexpr int cell(int s, int i) { return s ? i - i % W + (W - 1 - i % W) : i; }
    static constexpr int action(int s, int a) { return s ? W - 1 - a : a; }
    static constexpr int inverse(int s) { return s; }
    static constexpr int cell_inv(int s, int i) { return cell(inverse(s), i); }
    static constexpr int action_inv(int s, int a) { return action(inverse(s), a); }
};

template <> // BB_GAME_TICTACTOE
struct Symmetries<1> {
    static constexpr int H = 3, W = 3, A = 9, NSYM = 8;
    static constexpr int cell(int s, int i) {
        const int r = i / W, c = i % W;
        const int r1 = (s & 1) ? c : r, c1 = (s & 1) ? r : c;
        return ((s & 2) ? H - 1 - r1 : r1) * W + ((s & 4) ? W - 1 - c1 : c1);
    }
    static constexpr int action(int s, int a) { return cell(s, a); }
    // undoing "transpose, then the reversals" is "the reversals, then transpose" = "transpose, then the reversals swapped"
    static constexpr int inverse(int s) { return (s & 1) ? 1 | ((s & 2) << 1) | ((s & 4) >> 1) : s; }
    static constexpr int cell_inv(int s, int i) { return cell(inverse(s), i); }
    static constexpr int action_inv(int s, int a) { return action(inverse(s), a); }
};

template <> // BB_GAME_DRAGONCHESS
struct Symmetries<2> {
    static constexpr int H = 8, W = 8, A = 4032, NSYM = 1;
    static constexpr int cell(int, int i) { return i; }
    static constexpr int action(int, int a) { return a; }
    static constexpr int inverse(int s) { return s; }
    static constexpr int cell_inv(int, int i) { return i; }
    static constexpr int action_inv(int, int a) { return a; }
};

// the answer of bb_game_symmetries; -1: no such game
constexpr int game_symmetries(int game) {
    return game == 0 ? Symmetries<0>::NSYM : game == 1 ? Symmetries<1>::NSYM : game == 2 ? Symmetries<2>::NSYM : -1;
}
