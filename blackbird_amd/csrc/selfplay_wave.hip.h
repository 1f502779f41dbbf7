// selfplay_wave.hip.h -- self-play with the rollout evaluator (BB_EVAL_ROLLOUT through bb_selfplay_step) in ONE launch per call:
// one wave per game slot (opt-in: bb_selfplay_rollouts; bb_selfplay_mode 6).
//
// The lock-step structure pays sims_per_move x (k_tree_step + k_rollout) launches plus k_selfplay_move per ply, and every one of
// those simulations lasts as long as the longest playout among all slots.  The slots share nothing, so here a wave keeps its slot
// for whole plies, as the one-launch search does for one call of bb_run_sims (search_wave.hip.h, search_wave_dc.hip.h): per ply
// phase_apply -> phase_select -> the playout of the leaf in the slot's mailbox, `sims` times, then what k_selfplay_move does --
// the last phase_apply and selfplay_move_body: sample, record the example, re-root, and when the game is over hand the slot to its
// next game id.  No wave waits for another: no spin, no cross-wave synchronisation (the DragonChess kernel has the one barrier of
// its prologue); every loop is bounded by plies x sims, by H*W or by the 2048-ply cap of a DragonChess playout.
//
// Per slot this is exactly the lock-step sequence of operations -- run_sims(sims_now), then the move launch, `plies` times -- from
// the same device functions, with the draws keyed (game id, sim_serial - 1, 'ROLL', step) as k_rollout / k_dc_rollout key them, so
// records, headers, counters and the Philox stream are the lock-step ones byte for byte (tests/test_gpu_selfplay_wave_rollout.py).
// What ends a slot's loops early is what makes every further lock-step launch a no-op for it: a step that posts no leaf (no game,
// or no simulations left: nothing changes that before the move) ends the ply's simulations, and a slot without a game (it has
// played its last one: only its own move refills a slot) ends the call.
//
// `move` = 0 is the host's split of ONE ply that is longer than a launch may be (selfplay_wave_rollout, host_selfplay.hip.h): `sims` steps
// and no move, the last leaf stays pending in the mailbox exactly as it does between two lock-step launches, and the next launch's
// first phase_apply takes it.
#pragma once
#include "search_wave.hip.h"
#include "search_wave_dc.hip.h"

// Connect4 and TicTacToe.  A ply's simulations are sw_rollout_sims (search_wave.hip.h), the loop k_search_wave_rollout runs; the
// move's fences are those of k_selfplay_move; no LDS.  TreeDev stays a kernel argument (SGPRs) and every helper is inlined (see
// search_wave.hip.h).
template <class G>
__global__ void __launch_bounds__(64 * SW_WAVES) k_selfplay_wave_rollout(TreeDev d, int plies, int sims, int move) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = blockIdx.x * SW_WAVES + wave;
    if (g >= d.n_slots) return; // (whole waves leave: nothing here synchronises the workgroup)
    for (int p = 0; p < plies; p++) {
        if (__builtin_amdgcn_readfirstlane(d.game_lid[g]) < 0) break; // (uniform) the slot has played its last game
        sw_rollout_sims<G, true>(d, g, lane, sims);
        if (!move) break; // (uniform) part of a ply: the leaf stays pending for the next launch
        if (lane < G::S) { // k_selfplay_move
            phase_apply<G>(d, g, lane);
            __threadfence_block();
            selfplay_move_body<G>(d, g, lane);
        }
        __threadfence_block(); // lane 0's slot state (ply, sims_left, a new game's root) before the next ply's loads
    }
}

// DragonChess: a ply is the simulations of k_dc_search_wave_rollout -- its prologue, its out-of-line tree step and playout, the one
// set of instances the two kernels share (search_wave_dc.hip.h) -- and then dc_spw_move, out of line for the same reason (inlined
// into one loop body the phases spill: mega_dc.hip.h).
// k_dc_selfplay_move for the wave's slot (the body applies the last leaf first).  Returns the slot's game (wave-uniform; < 0: none).
__device__ __attribute__((noinline)) int dc_spw_move(const TreeDev &d_, const DCEdges &E_, int g, int lane, float *tl) {
    const TreeDev &d = *as_lds(&d_);
    const DCEdges &E = *as_lds(&E_);
    dc_selfplay_move_body<DC_COPY_ROLLOUT_WAVE>(d, E, g, lane, as_lds(tl));
    __threadfence_block(); // lane 0's slot state (ply, sims_left, a new game's root) before the next ply's loads
    return __builtin_amdgcn_readfirstlane(as_global(d.game_lid)[g]);
}
__global__ void __launch_bounds__(64 * SW_WAVES) k_dc_selfplay_wave_rollout(TreeDev d_arg, DCEdges E_arg, int plies, int sims, int move) {
    const DCRolloutWave w = dc_swr_prologue(d_arg, E_arg);
    if (w.g < 0) return;
    if (__builtin_amdgcn_readfirstlane(d_arg.game_lid[w.g]) < 0) return; // (uniform) the slot has played its last game
    for (int p = 0; p < plies; p++) {
        dc_swr_sims(w, sims);
        if (!move) break; // (uniform) part of a ply: the leaf stays pending for the next launch
        if (dc_spw_move(*w.d, *w.E, w.g, w.lane, w.tl) < 0) break; // (uniform) that was the slot's last game
    }
}
