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
// `move` = 0 is the host's split of ONE ply that is longer than a launch may be (selfplay_wave_rollout, engine.hip): `sims` steps
// and no move, the last leaf stays pending in the mailbox exactly as it does between two lock-step launches, and the next launch's
// first phase_apply takes it.
#pragma once
#include "search_wave.hip.h"
#include "search_wave_dc.hip.h"

// Connect4 and TicTacToe.  The fences are those of k_search_wave_rollout and k_selfplay_move; no LDS.  TreeDev stays a kernel
// argument (SGPRs) and every helper is inlined (see search_wave.hip.h).
template <class G>
__global__ void __launch_bounds__(64 * SW_WAVES) k_selfplay_wave_rollout(TreeDev d, int plies, int sims, int move) {
    constexpr int S = G::S;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = blockIdx.x * SW_WAVES + wave;
    if (g >= d.n_slots) return; // (whole waves leave: nothing here synchronises the workgroup)
    const bool tree_lane = lane < S;
    for (int p = 0; p < plies; p++) {
        if (__builtin_amdgcn_readfirstlane(d.game_lid[g]) < 0) break; // (uniform) the slot has played its last game
        for (int s = 0; s < sims; s++) {
            if (tree_lane) {
                phase_apply<G>(d, g, lane);
                __threadfence_block();
                phase_select<G>(d, g, lane);
            }
            __threadfence_block(); // lane 0's mailbox stores before the other lanes' loads
            if (__builtin_amdgcn_readfirstlane(d.pend_leaf[g]) < 0) break; // (uniform) nothing posted: every further step is a no-op
            const typename G::State st = ((const typename G::State *)d.leaf_state)[g];
            const uint32_t gid = (uint32_t)__builtin_amdgcn_readfirstlane((int)d.leaf_game_id[g]);
            const uint32_t serial = (uint32_t)(__builtin_amdgcn_readfirstlane(d.sim_serial[g]) - 1);
            const float v = rollout_value_wave<G>(st, d.seed, gid, serial, lane);
            if (lane == 0) d.eval_value[g] = v;
            __threadfence_block(); // the value is in the mailbox before phase_apply reads it
        }
        if (!move) break; // (uniform) part of a ply: the leaf stays pending for the next launch
        if (tree_lane) { // k_selfplay_move
            phase_apply<G>(d, g, lane);
            __threadfence_block();
            selfplay_move_body<G>(d, g, lane);
        }
        __threadfence_block(); // lane 0's slot state (ply, sims_left, a new game's root) before the next ply's loads
    }
}

// DragonChess: the same loop with dc_phase_apply / dc_phase_select / dc_rollout_wave / dc_selfplay_move_body, on the per-wave tree
// scratch and the LDS copies of the descriptors as in k_dc_search_wave_rollout.  The phases are out of line (inlined into one loop
// body they spill: mega_dc.hip.h) and instances of this kernel alone (COPY = 2), so the existing kernels are compiled as they were.
// Self-play refuses track_ancestors engines, so the tree step's ancestor walk (ANC, as k_dc_tree_step) finds no chain.
// Returns the posted leaf (wave-uniform; < 0: none).
__device__ __attribute__((noinline)) int dc_spw_tree(const TreeDev &d_, const DCEdges &E_, int g, int lane, float *tl) {
    const TreeDev &d = *as_lds(&d_);
    const DCEdges &E = *as_lds(&E_);
    tl = as_lds(tl);
    dc_phase_apply<false, true, 2>(d, E, g, lane, tl);
    __threadfence_block();
    dc_phase_select<false, 2>(d, E, g, lane, tl);
    __threadfence_block(); // lane 0's mailbox stores before the other lanes' loads
    return __builtin_amdgcn_readfirstlane(as_global(d.pend_leaf)[g]);
}
__device__ __attribute__((noinline)) void dc_spw_rollout(const TreeDev &d_, int g, int lane) {
    const TreeDev &d = *as_lds(&d_);
    const uint32_t gid = (uint32_t)__builtin_amdgcn_readfirstlane((int)as_global(d.leaf_game_id)[g]);
    const uint32_t serial = (uint32_t)(__builtin_amdgcn_readfirstlane(as_global(d.sim_serial)[g]) - 1);
    const float v = dc_rollout_wave(as_global((const DCState *)d.leaf_state) + g, gid, serial, d.seed, lane);
    if (lane == 0) as_global(d.eval_value)[g] = v;
    __threadfence_block(); // the value is in the mailbox before dc_phase_apply reads it
}
// k_dc_selfplay_move for the wave's slot (the body applies the last leaf first).  Returns the slot's game (wave-uniform; < 0: none).
__device__ __attribute__((noinline)) int dc_spw_move(const TreeDev &d_, const DCEdges &E_, int g, int lane, float *tl) {
    const TreeDev &d = *as_lds(&d_);
    const DCEdges &E = *as_lds(&E_);
    dc_selfplay_move_body<2>(d, E, g, lane, as_lds(tl));
    __threadfence_block(); // lane 0's slot state (ply, sims_left, a new game's root) before the next ply's loads
    return __builtin_amdgcn_readfirstlane(as_global(d.game_lid)[g]);
}
__global__ void __launch_bounds__(64 * SW_WAVES) k_dc_selfplay_wave_rollout(TreeDev d_arg, DCEdges E_arg, int plies, int sims, int move) {
    __shared__ __attribute__((aligned(16))) float lds_all[SW_WAVES][DC_LDS_FLOATS];
    __shared__ TreeDev s_d;
    __shared__ DCEdges s_E;
    if (threadIdx.x == 0) { // workgroup prologue: the one barrier of the kernel
        s_d = d_arg;
        s_E = E_arg;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int g = blockIdx.x * SW_WAVES + wv;
    if (g >= d_arg.n_slots) return; // (whole waves leave: nothing below synchronises the workgroup)
    float *tl = lds_all[wv];
    if (__builtin_amdgcn_readfirstlane(d_arg.game_lid[g]) < 0) return; // (uniform) the slot has played its last game
    for (int p = 0; p < plies; p++) {
        for (int s = 0; s < sims; s++) {
            if (dc_spw_tree(s_d, s_E, g, lane, tl) < 0) break; // (uniform) no simulations left: every further step is a no-op
            dc_spw_rollout(s_d, g, lane);
        }
        if (!move) break; // (uniform) part of a ply: the leaf stays pending for the next launch
        if (dc_spw_move(s_d, s_E, g, lane, tl) < 0) break; // (uniform) that was the slot's last game
    }
}
