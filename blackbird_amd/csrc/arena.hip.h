// arena.hip.h -- the match loop of Blackbird.TestModels (Blackbird.py:177-216) on the device: what the arena keeps per game and the
// two small kernels that stand where the host loop of blackbird_amd/arena.py reads results back.  Everything that touches a search
// tree is an existing launch of the two engines (set_roots, k_add_sims, the search, sample, move_roots: host_arena.hip.h enqueues them on
// the engines' own streams); the kernels here only read the engines' out_action rows and write the arena's own arrays, which are
// then the arguments of those launches.  One thread per slot, plain stores: a game is owned by one thread.
#pragma once
#include "games.hip.h"

// error word of a game (0: none); the game stops where it is set
#define BB_ARENA_ERR_ILLEGAL (-100) // G::apply refused the chosen action ('Tried to make an illegal move.')

struct ArenaDev {
    int n_slots, n_games, log_plies;
    void *states;          // [n_slots] packed current state of game i
    uint8_t *a_to_move;    // [n_slots] engine a is the mover of game i's next ply
    uint8_t *a_player;     // [n_slots] the player number a was given: 1 if it moved first, else 2
    uint8_t *alive;        // [n_slots] 0: finished, stopped by an error, or no game in this slot
    uint8_t *primed_a, *primed_b; // [n_slots] the side's slot i holds a tree of this game (FindMove's `Root is None` branch was taken)
    int8_t *result;        // [n_slots] +1 / 0 / -1 from a's point of view
    int32_t *plies;        // [n_slots] moves made
    int32_t *err;          // [n_slots] the negative action bb_sample_moves would have reported (-4: NaN probabilities), or BB_ARENA_ERR_ILLEGAL
    int32_t *log;          // [n_slots][log_plies] actions, -1 padded
    uint8_t *mask_a, *mask_b;     // [n_slots] k_add_sims' mask of this ply, per side
    int32_t *prime_a, *prime_b;   // [n_slots] set_roots' slot list of this ply: i where the side is to be primed, else -1 (skipped)
    int32_t *mv_a, *mv_b;         // [n_slots] move_roots' actions of this ply: -1 leaves the slot alone
    uint32_t *gids;        // [n_slots] game id of slot i: i
};

// Steps 1-2 of a ply (arena.py:92-106): who searches, and which slots are primed first.
__global__ void __launch_bounds__(256) k_arena_prep(ArenaDev ar) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ar.n_slots) return;
    const bool live = i < ar.n_games && ar.alive[i];
    const bool ma = live && ar.a_to_move[i], mb = live && !ar.a_to_move[i];
    ar.mask_a[i] = ma;
    ar.mask_b[i] = mb;
    ar.prime_a[i] = ma && !ar.primed_a[i] ? i : -1;
    ar.prime_b[i] = mb && !ar.primed_b[i] ? i : -1;
    if (ma) ar.primed_a[i] = 1;
    if (mb) ar.primed_b[i] = 1;
}

// Steps 4-8 of a ply (arena.py:113-133) once both sides' sample launches have written their out_action rows: the mover's action,
// the move on the arena's state, the log, what each primed side's MoveRoot gets, Winner() with no previous action, the turn.
template <class G>
__global__ void __launch_bounds__(256) k_arena_move(ArenaDev ar, const int32_t *out_a, const int32_t *out_b) {
    using State = typename G::State;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ar.n_slots) return;
    ar.mv_a[i] = -1;
    ar.mv_b[i] = -1;
    if (i >= ar.n_games || !ar.alive[i]) return;
    const bool am = ar.a_to_move[i] != 0;
    const int act = am ? out_a[i] : out_b[i];
    if (act < 0 || act >= G::A) { // bb_sample_moves' negative answers: 'probabilities contain NaN'
        ar.err[i] = act < 0 ? act : BB_ARENA_ERR_ILLEGAL;
        ar.alive[i] = 0;
        return;
    }
    State *sp = (State *)ar.states + i;
    State s = *sp;
    if (!G::apply(s, act)) {
        ar.err[i] = BB_ARENA_ERR_ILLEGAL;
        ar.alive[i] = 0;
        return;
    }
    *sp = s;
    const int p = ar.plies[i];
    if (p < ar.log_plies) ar.log[(size_t)i * ar.log_plies + p] = act;
    ar.plies[i] = p + 1;
    if (ar.primed_a[i]) ar.mv_a[i] = act;
    if (ar.primed_b[i]) ar.mv_b[i] = act;
    const int w = G::winner(s, -1);
    if (w >= 0) {
        ar.alive[i] = 0;
        ar.result[i] = (int8_t)(w == 0 ? 0 : (w == (int)ar.a_player[i] ? 1 : -1));
    }
    ar.a_to_move[i] = am ? 0 : 1; // the callers of FindMove alternate every ply, whatever state.Player says (Blackbird.py:196-201)
}
