// search_wave.hip.h -- the search API (bb_run_sims / bb_run_sims_masked) in ONE launch: one wave per game slot.
//
// The lock-step search is a host loop of two launches per simulation (k_tree_step, then the evaluator over every slot): a
// lone FindMove position pays 2 x 800 launches per move, and so does every ply of an arena however few games it plays.
// The slots share nothing, so here a wave keeps its slot for the whole call, as k_dc_selfplay_fused does for DragonChess
// self-play (mega_dc.hip.h): phase_apply -> phase_select -> the evaluator for its own leaf -> ..., and after the last
// simulation the pending evaluation is applied (what Launch<G>::tree_apply does for the lock-step loop), so nothing
// outlives the launch.  No wave waits for another: no spin, no cross-wave synchronisation, every loop is bounded by `sims`.
//
// Per slot this is exactly the lock-step sequence of operations, from the same device functions -- phase_apply /
// phase_select (tree.hip.h: backup_path with the ancestor walk of track_anc engines, terminal leaves, a full node pool ->
// the overflow counter, slots without sims_left), then what k_hash_eval or k_net_x3 do for one slot: net_body_x3 on the leaf in
// the slot's mailbox with the prior noise keyed (game id, node serial, action) -- so trees, counters and sampled moves are
// the lock-step ones bit for bit (tests/test_gpu_search_wave.py).  One difference nobody can observe: the lock-step
// evaluator launch also rewrites the mailboxes of slots that posted nothing; here an idle slot's mailbox is left alone.
//
// The tree phases run on lanes 0 .. S-1, the network on all 64; what decides whether the network runs is made
// wave-uniform (readfirstlane), so net_body_x3 is never entered with part of the wave masked off.  TreeDev stays a kernel
// argument (SGPRs) and every helper is inlined: an out-of-line callee would take it by reference from scratch.
#pragma once
#include "eval.hip.h"
#include "net_x3.hip.h"
#include "tree.hip.h"

#define SW_WAVES 4 // waves (= slots) per workgroup: four waves' activations (X3Geom::WAVE_BYTES each) as in k_net_x3, one wave per SIMD

// what k_hash_eval does for position g of the leaf mailbox: every lane forms the hash, lane a writes action a
template <class G>
__device__ __forceinline__ void sw_hash_eval(const TreeDev &d, int g, int lane) {
    const typename G::State st = ((const typename G::State *)d.leaf_state)[g];
    const uint64_t sl = d.salt + (d.salt_per_game ? (uint64_t)(d.leaf_game_id[g] - d.first_game_id) : 0ull);
    const uint64_t z = hash_state<G>(st, sl);
    if (lane == 0) d.eval_value[g] = bb_hash_value(z);
    if (lane < G::A) d.eval_policy[(size_t)g * G::S + lane] = bb_hash_policy(z, lane);
}

// NET: the 16-filter network in the split-operand form (x3.w0 set); else the hash evaluator.
// CACHE (bb_config.search_cache, an engine that owns a table; Connect4 with NET): the leaf's entry of the engine's evaluation cache
// (net.hip.h) is requested before the network's prologue and tested after it, as in the persistent self-play kernel (mega2.hip.h).  A
// hit runs only dense_prior_tail on the cached value and pre-noise priors, with the node's own noise key (game id, node serial,
// action), so it leaves in the mailbox the bits the tower would have; a miss stores from head_one into the way the probe picked.
// d.evals keeps counting tower runs: phase_select counted the leaf when it posted it, a hit takes it back.  The wave counts its
// probes and hits in registers and adds them to the engine's counters once, from one lane.  Two waves that evaluate one position at
// the same time both miss and both store the same bits (the entry protocol of net.hip.h): nobody waits for anybody.
template <class G, bool NET, bool CACHE = false>
__global__ void __launch_bounds__(64 * SW_WAVES) k_search_wave(TreeDev d, NetDev nd, NetX3 x3, int sims, int noise) {
    using XG = X3Geom<G>;
    constexpr int S = G::S;
    static_assert(!CACHE || (NET && G::CACHE_KEY), "the evaluation cache: the network's evaluations of a game with a one-word key");
    __shared__ __attribute__((aligned(16))) unsigned char lds[NET ? SW_WAVES * XG::WAVE_BYTES : 16];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = blockIdx.x * SW_WAVES + wave;
    if (g >= d.n_slots) return; // (whole waves leave: nothing below synchronises the workgroup)
    const bool tree_lane = lane < S;
    unsigned n_probes = 0, n_hits = 0; // (CACHE) this wave's call
    (void)n_probes;
    (void)n_hits;
    for (int s = 0; s < sims; s++) { // the lock-step loop's `sims` steps, for this slot
        if (tree_lane) {
            phase_apply<G>(d, g, lane);
            __threadfence_block();
            phase_select<G>(d, g, lane);
        }
        __threadfence_block(); // lane 0's mailbox stores before the other lanes' loads
        // (uniform) no leaf posted: the slot is idle, masked out or out of simulations, and every further step is a no-op
        if (__builtin_amdgcn_readfirstlane(d.pend_leaf[g]) < 0) break;
        if constexpr (CACHE) {
            int probe = -1;
            net_body_x3<G, false, false, true>(nd, x3, g + 1, g, nullptr, lds + wave * XG::WAVE_BYTES, (const typename G::State *)d.leaf_state, nullptr,
                                               d.leaf_game_id, d.leaf_serial, noise, d.eval_value, nullptr, d.eval_policy, S, true, nullptr,
                                               EvalCache{(u32x4 *)d.eval_cache, d.eval_cache_log2}, &probe);
            n_probes += probe >= 0;
            if (probe > 0) {
                n_hits++;
                if (lane == 0) d.evals[g] -= 1;
            }
        } else if constexpr (NET)
            net_body_x3<G, false>(nd, x3, g + 1, g, nullptr, lds + wave * XG::WAVE_BYTES, (const typename G::State *)d.leaf_state, nullptr,
                                  d.leaf_game_id, d.leaf_serial, noise, d.eval_value, nullptr, d.eval_policy, S, true);
        else
            sw_hash_eval<G>(d, g, lane);
        __threadfence_block(); // the evaluation is in the mailbox before phase_apply reads it
    }
    if (tree_lane) phase_apply<G>(d, g, lane); // the last simulation's evaluation (no-op without a pending leaf)
    if constexpr (CACHE) {
        if (lane == 0 && n_probes && d.eval_cache_ctr) {
            atomicAdd(&d.eval_cache_ctr[0], (unsigned long long)n_hits);
            atomicAdd(&d.eval_cache_ctr[1], (unsigned long long)n_probes);
        }
    }
}

// ---- the rollout evaluator (BB_EVAL_ROLLOUT: MCTS.SampleValue, what k_rollout does for one slot) ----------------------------------
// The playout of rollout_value (eval.hip.h) by a whole wave.  Its Philox calls are the bulk of the arithmetic and do not depend on the
// position: a playout of a dense game has at most H*W steps, so lane k computes step k's draw once, up front, and the serial play
// loop takes step k's draw from lane k.  The position is wave-uniform (scalar registers), so the loop is scalar arithmetic plus one
// v_readlane per step.  The same draws on the same positions in the same order as rollout_value: the same value, bit for bit.
template <class G>
__device__ __forceinline__ float rollout_value_wave(typename G::State s, uint64_t seed, uint32_t game_id, uint32_t serial, int lane) {
    static_assert(G::H * G::W <= 64, "one lane per step of the longest playout");
    s.p1 = ((uint64_t)__builtin_amdgcn_readfirstlane((int)(s.p1 >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)s.p1);
    s.p2 = ((uint64_t)__builtin_amdgcn_readfirstlane((int)(s.p2 >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)s.p2);
    const int player = gs_prev(s);
    int w = G::winner(s, -1);
    if (w < 0) { // (uniform) a leaf that is already decided draws nothing
        const uint32_t draw = philox4x32_10(seed, game_id, serial, BB_TAG_ROLL, (uint32_t)lane).x[0];
        for (int step = 0; w < 0 && step < G::H * G::W; step++) { // (every step puts a stone on the board)
            const uint32_t m = G::legal_mask(s);
            const int cnt = __popc(m);
            const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)draw, step);
            int pick = (int)(((uint64_t)r0 * (uint64_t)cnt) >> 32);
            uint32_t mm = m;
            for (; pick > 0; pick--) mm &= mm - 1; // the pick-th legal move in ascending order
            const int a = mm ? __builtin_ctz(mm) : 0;
            G::apply(s, a);
            w = G::winner(s, a);
        }
    }
    return w == 0 ? 0.5f : (player == w ? 1.0f : 0.0f);
}

// Up to `sims` simulations of slot g with the rollout evaluator: phase_apply -> phase_select -> the playout of the leaf in the slot's
// mailbox -> ...; the last leaf stays pending, as between two lock-step launches.  THE simulation loop of both rollout wave kernels
// of the dense games (k_search_wave_rollout below, k_selfplay_wave_rollout in selfplay_wave.hip.h), inlined into each.
// The draws are keyed (game id, sim_serial - 1, 'ROLL', step) with sim_serial read after phase_select has advanced it -- what
// k_rollout reads in the lock-step loop -- so the trees are the lock-step ones bit for bit (tests/test_gpu_search_wave_rollout.py).
// LANES: rollout_value_wave; else lane 0 runs rollout_value, literally k_rollout's thread (the form the other was measured against).
template <class G, bool LANES>
__device__ __forceinline__ void sw_rollout_sims(const TreeDev &d, int g, int lane, int sims) {
    const bool tree_lane = lane < G::S;
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
        if constexpr (LANES) {
            const float v = rollout_value_wave<G>(st, d.seed, gid, serial, lane);
            if (lane == 0) d.eval_value[g] = v;
        } else {
            if (lane == 0) d.eval_value[g] = rollout_value<G>(st, d.seed, gid, serial);
        }
        __threadfence_block(); // the value is in the mailbox before phase_apply reads it
    }
}

// k_search_wave with the rollout evaluator: the simulations above and the last simulation's apply.  A kernel of its own, so the hash
// and network instantiations above are compiled as they were; no LDS.
template <class G, bool LANES>
__global__ void __launch_bounds__(64 * SW_WAVES) k_search_wave_rollout(TreeDev d, int sims) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = blockIdx.x * SW_WAVES + wave;
    if (g >= d.n_slots) return; // (whole waves leave: nothing here synchronises the workgroup)
    sw_rollout_sims<G, LANES>(d, g, lane, sims);
    if (lane < G::S) phase_apply<G>(d, g, lane); // the last simulation's evaluation (no-op without a pending leaf)
}
