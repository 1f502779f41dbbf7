// search_wave_dc.hip.h -- the search API (bb_run_sims / bb_run_sims_masked) of a DragonChess engine in ONE launch: one wave per slot.
//
// What search_wave.hip.h is for the dense games, in the shape k_dc_selfplay_fused (mega_dc.hip.h) gives the wide one: a wave keeps its
// slot for the whole call -- dc_phase_apply (with the ancestor walk: FindMove engines track their ancestors) -> dc_phase_select -> the
// network for its own leaf on the bf16 matrix pipe -> ..., `sims` times, then the pending evaluation is applied (what k_dc_tree_apply
// does for the lock-step loop), so nothing outlives the launch.  No move kernel, no pool of simulations; the evaluation-cache probe is
// the CACHE instantiation (bb_config.search_cache, below).  Nothing 4032-wide leaves the wave: the policy head is reduced to five numbers (WideHead) in LDS and
// the expansion forms the priors of the legal moves only, from the head weights in LDS -- the same operations on the same inputs
// as the 16 KB row k_net_x3 writes and dc_expand gathers from, so the same bits (tests/test_gpu_search_wave_dc.py; the self-play
// kernel is held to that by tests/test_gpu_mcts.py).  No wave waits for another: no spin, every loop is bounded by `sims`.
//
// The control state (TreeDev's per-slot arrays, the paths, the ancestor chain) stays in HBM: that is the instantiation of the tree
// phases the ancestor walk exists for (dc_phase_apply<false, true>, as k_dc_tree_step).  The one thing copied is the posted leaf's
// position, 80 bytes into LDS, because the two-buffer network reads its input there.
//
// When does a slot stop early?  dc_phase_select posts a leaf whenever it descends at all -- a terminal leaf, a full node or edge pool
// (the parent stands in, the overflow counter counts) and a path at MAXPATH all post -- and returns without posting only for a slot
// without a game (game_lid < 0) or without simulations left (sims_left <= 0: masked out, or nothing added).  Neither changes inside a
// call, the apply before it has cleared pend_leaf, so every further lock-step step is a no-op for the slot: that, and only that, ends
// the loop before `sims`.
#pragma once
#include "mega_dc.hip.h"
#include "search_wave.hip.h"

// The phases are out of line for the reason given in mega_dc.hip.h (inlined into one loop body they spill), and reach the kernel's
// descriptors through its LDS copies.  Returns the posted leaf (wave-uniform; < 0: none), its position copied to *leaf.
__device__ __attribute__((noinline)) int dc_sw_tree(const TreeDev &d_, const DCEdges &E_, int g, int lane, float *tl, const DCHeadLocal *hl, DCState *leaf) {
    const TreeDev &d = *as_lds(&d_);
    const DCEdges &E = *as_lds(&E_);
    tl = as_lds(tl);
    leaf = as_lds(leaf);
    hl = as_lds(hl);
    dc_phase_apply<false, true>(d, E, g, lane, tl, hl);
    __threadfence_block();
    dc_phase_select<false>(d, E, g, lane, tl);
    __threadfence_block(); // lane 0's mailbox stores before the other lanes' loads
    const int posted = __builtin_amdgcn_readfirstlane(as_global(d.pend_leaf)[g]);
    if (posted >= 0 && lane < (int)(sizeof(DCState) / 4)) ((uint32_t *)leaf)[lane] = ((const uint32_t *)(as_global((const DCState *)d.leaf_state) + g))[lane];
    __threadfence_block();
    return posted;
}
__device__ __attribute__((noinline)) void dc_sw_apply(const TreeDev &d_, const DCEdges &E_, int g, int lane, float *tl, const DCHeadLocal *hl) {
    const TreeDev &d = *as_lds(&d_);
    const DCEdges &E = *as_lds(&E_);
    tl = as_lds(tl);
    hl = as_lds(hl);
    dc_phase_apply<false, true>(d, E, g, lane, tl, hl);
    __threadfence_block();
}
// The network for the wave's own leaf (dc_fused_net_x3 without the cache probe): position *slot of `leaf`, both in LDS.
__device__ __forceinline__ void dc_sw_net(const NetDev &nd_, const NetX3 &x3_, const DCState *leaf, const int *slot, float *nl, DCHeadLocal *hl) {
    const NetDev &nd = *as_lds(&nd_);
    const NetX3 &x3 = *as_lds(&x3_);
    slot = as_lds(slot);
    nl = as_lds(nl);
    hl = as_lds(hl);
    // (noise 0: a wide game's prior noise is mixed in at expansion, E.noise_on; the compact form writes nothing but hl->h)
    net_body_x3<DragonChess, false, true>(nd, x3, 1, 0, slot, (unsigned char *)nl, leaf, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                                          DragonChess::A, true, &hl->h);
    __threadfence_block();
}
// The same behind the evaluation cache (bb_config.search_cache, an engine that owns a table; what dc_fused_net_x3 is to the
// self-play kernel): the leaf's entry is probed first, with the key formed from the wave's LDS copy of the leaf (dc_leaf_probe,
// mega_dc.hip.h).  A hit puts the cached WideHead in hl->h, takes the leaf back from d.evals and skips the network; a miss stores
// the WideHead the network leaves.  The entry is pre-noise, as in self-play: a wide game's prior noise is mixed in at expansion.
// Returns what dc_leaf_probe does: -1 no probe (a state without a key), 0 miss, 1 hit.
__device__ __forceinline__ int dc_sw_net_cached(const NetDev &nd_, const NetX3 &x3_, const TreeDev &d_, int g, const DCState *leaf, const int *slot,
                                                float *nl, DCHeadLocal *hl) {
    const TreeDev &d = *as_lds(&d_);
    const DCState *mine = as_lds(leaf) + *as_lds(slot);
    const int lane = threadIdx.x & 63;
    const int probe = dc_leaf_probe(d, mine, g, as_lds(hl), lane);
    if (probe > 0) return probe;
    dc_sw_net(nd_, x3_, leaf, slot, nl, hl);
    if (probe == 0) {
        dc_leaf_store(d, mine, as_lds(hl), lane);
        __threadfence_block();
    }
    return probe;
}

// host: 16-filter network in the split-operand form, nd.R <= DC_RMAX, nd.head_floats <= DC_HEAD_FLOATS (search_structure)
template <bool CACHE>
__device__ __forceinline__ void dc_search_wave_body(const TreeDev &d_arg, const DCEdges &E_arg, const NetDev &nd_arg, const NetX3 &x3_arg, int sims) {
    // the tree's scratch (the 4032-float policy image) and the network's activations are never live together
    constexpr int TREE_BYTES = DC_LDS_FLOATS * 4, NET_BYTES = X3Geom<DragonChess>::WAVE_BYTES_PP;
    constexpr int WAVE_BYTES = ((TREE_BYTES > NET_BYTES ? TREE_BYTES : NET_BYTES) + 15) / 16 * 16;
    static_assert(SW_WAVES * WAVE_BYTES + DC_HEAD_FLOATS * 4 + DC_EPI_FLOATS * 4 + 2048 <= 163840, "the waves' scratch and the head weights must fit the 160 KiB LDS");
    __shared__ __attribute__((aligned(16))) unsigned char lds_all[SW_WAVES][WAVE_BYTES];
    __shared__ __attribute__((aligned(16))) float s_head[DC_HEAD_FLOATS];
    __shared__ __attribute__((aligned(16))) float s_epi[DC_EPI_FLOATS];
    __shared__ __attribute__((aligned(16))) DCState s_leaf[SW_WAVES];
    __shared__ int myslot[SW_WAVES];
    __shared__ DCHeadLocal s_hl[SW_WAVES];
    __shared__ TreeDev s_d;
    __shared__ DCEdges s_E;
    __shared__ NetDev s_nd;
    __shared__ NetX3 s_x3;
    // workgroup prologue, all four waves: the one barrier of the kernel
    for (int i = threadIdx.x; i < nd_arg.head_floats; i += blockDim.x) s_head[i] = nd_arg.head[i];
    for (int i = threadIdx.x; i < 48 * (1 + 2 * nd_arg.R); i += blockDim.x) s_epi[i] = nd_arg.epi[i];
    if (threadIdx.x == 0) {
        s_d = d_arg;
        s_E = E_arg;
        s_nd = nd_arg;
        s_nd.head = s_head;
        s_nd.epi = s_epi;
        s_x3 = x3_arg;
    }
    if (threadIdx.x < SW_WAVES) {
        using LP = const __attribute__((address_space(3))) float *;
        s_hl[threadIdx.x].pdk = (LP)s_head + nd_arg.off_pdk;
        s_hl[threadIdx.x].pdb = (LP)s_head + nd_arg.off_pdb;
        s_hl[threadIdx.x].h = WideHead{0.f, 0.f, 0.f, 0.f, 0.f};
        myslot[threadIdx.x] = threadIdx.x; // the wave's position in s_leaf
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int g = blockIdx.x * SW_WAVES + wv;
    if (g >= d_arg.n_slots) return; // (whole waves leave: nothing below synchronises the workgroup)
    float *tl = (float *)lds_all[wv];
    DCHeadLocal *hl = &s_hl[wv];
    // (no leaf is pending on entry: every entry point that searches -- this kernel, the lock-step loop, the self-play structures --
    // applies its last evaluation before it returns)
    bool pending = false;
    [[maybe_unused]] unsigned n_probes = 0, n_hits = 0; // (CACHE) this wave's call: one counter update at the end
    for (int s = 0; s < sims; s++) { // the lock-step loop's `sims` steps, for this slot
        pending = dc_sw_tree(s_d, s_E, g, lane, tl, hl, &s_leaf[wv]) >= 0;
        if (!pending) break; // (uniform) no game or no simulations left: every further step is a no-op (see the head of this file)
        if constexpr (CACHE) {
            const int probe = dc_sw_net_cached(s_nd, s_x3, s_d, g, s_leaf, &myslot[wv], tl, hl);
            n_probes += probe >= 0;
            n_hits += probe > 0;
        } else
            dc_sw_net(s_nd, s_x3, s_leaf, &myslot[wv], tl, hl);
    }
    if (pending) dc_sw_apply(s_d, s_E, g, lane, tl, hl); // the last simulation's evaluation
    if constexpr (CACHE) {
        if (lane == 0 && n_probes && d_arg.eval_cache_ctr) {
            atomicAdd(&d_arg.eval_cache_ctr[0], (unsigned long long)n_hits);
            atomicAdd(&d_arg.eval_cache_ctr[1], (unsigned long long)n_probes);
        }
    }
}
// (Two kernels that call the same out-of-line phases: beside the second one, the first is compiled with one spilled scalar register
// where alone it has none; every other figure of it is unchanged.  Copies of the phases per kernel -- plain or as template instances --
// cost both kernels two accumulator registers and 8 bytes of scratch instead.)
__global__ void __launch_bounds__(64 * SW_WAVES) k_dc_search_wave(TreeDev d_arg, DCEdges E_arg, NetDev nd_arg, NetX3 x3_arg, int sims) {
    dc_search_wave_body<false>(d_arg, E_arg, nd_arg, x3_arg, sims);
}
// ... behind the evaluation cache (bb_config.search_cache, an engine that owns a table)
__global__ void __launch_bounds__(64 * SW_WAVES) k_dc_search_wave_cached(TreeDev d_arg, DCEdges E_arg, NetDev nd_arg, NetX3 x3_arg, int sims) {
    dc_search_wave_body<true>(d_arg, E_arg, nd_arg, x3_arg, sims);
}

// ---- the rollout evaluator (BB_EVAL_ROLLOUT) ------------------------------------------------------------------------------------------
// The same loop with dc_rollout_wave (tree_dc.hip.h: the body of k_dc_rollout) in the network's place: dc_phase_apply<false, true> ->
// dc_phase_select -> the playout of the leaf in the slot's mailbox -> ..., then the last apply.  Uniform priors are set at expansion
// (d.priors_ones), the value travels through d.eval_value[g] as in the lock-step loop (no DCHeadLocal), and the draws are keyed (game
// id, sim_serial - 1, 'ROLL', step) with sim_serial read after dc_phase_select has advanced it: what k_dc_rollout reads, so the same
// trees bit for bit (tests/test_gpu_search_wave_rollout.py).  None of the network's LDS: the tree's per-wave scratch and the
// descriptor copies only.
// The helpers below -- tree step, playout, last apply -- and the workgroup prologue serve BOTH rollout wave kernels: this one and
// k_dc_selfplay_wave_rollout (selfplay_wave.hip.h), whose ply is this kernel's simulation loop and then a move.  The phases are
// out of line and one set of instances for the two (DC_COPY_ROLLOUT_WAVE, tree_dc.hip.h), apart from those of the kernels above.
// Self-play refuses track_ancestors engines, so there the tree step's ancestor walk (ANC, as k_dc_tree_step) finds no chain.
// Returns the posted leaf (wave-uniform; < 0: none).
__device__ __attribute__((noinline)) int dc_swr_tree(const TreeDev &d_, const DCEdges &E_, int g, int lane, float *tl) {
    const TreeDev &d = *as_lds(&d_);
    const DCEdges &E = *as_lds(&E_);
    tl = as_lds(tl);
    dc_phase_apply<false, true, DC_COPY_ROLLOUT_WAVE>(d, E, g, lane, tl);
    __threadfence_block();
    dc_phase_select<false, DC_COPY_ROLLOUT_WAVE>(d, E, g, lane, tl);
    __threadfence_block(); // lane 0's mailbox stores before the other lanes' loads
    return __builtin_amdgcn_readfirstlane(as_global(d.pend_leaf)[g]);
}
__device__ __attribute__((noinline)) void dc_swr_apply(const TreeDev &d_, const DCEdges &E_, int g, int lane, float *tl) {
    const TreeDev &d = *as_lds(&d_);
    const DCEdges &E = *as_lds(&E_);
    dc_phase_apply<false, true, DC_COPY_ROLLOUT_WAVE>(d, E, g, lane, as_lds(tl));
    __threadfence_block();
}
__device__ __attribute__((noinline)) void dc_swr_rollout(const TreeDev &d_, int g, int lane) {
    const TreeDev &d = *as_lds(&d_);
    const uint32_t gid = (uint32_t)__builtin_amdgcn_readfirstlane((int)as_global(d.leaf_game_id)[g]);
    const uint32_t serial = (uint32_t)(__builtin_amdgcn_readfirstlane(as_global(d.sim_serial)[g]) - 1);
    const float v = dc_rollout_wave(as_global((const DCState *)d.leaf_state) + g, gid, serial, d.seed, lane);
    if (lane == 0) as_global(d.eval_value)[g] = v;
    __threadfence_block(); // the value is in the mailbox before dc_phase_apply reads it
}
// The workgroup prologue of a rollout wave kernel: the descriptors copied to LDS behind the one barrier of the kernel, then the
// wave's lane, slot and tree scratch.  g < 0: a wave beyond n_slots, which leaves (nothing after the prologue synchronises the
// workgroup).
struct DCRolloutWave {
    const TreeDev *d; // the LDS copies, as the out-of-line helpers take them
    const DCEdges *E;
    float *tl;
    int g, lane;
};
__device__ __forceinline__ DCRolloutWave dc_swr_prologue(const TreeDev &d_arg, const DCEdges &E_arg) {
    __shared__ __attribute__((aligned(16))) float lds_all[SW_WAVES][DC_LDS_FLOATS];
    __shared__ TreeDev s_d;
    __shared__ DCEdges s_E;
    if (threadIdx.x == 0) {
        s_d = d_arg;
        s_E = E_arg;
    }
    __syncthreads();
    const int wv = threadIdx.x >> 6, g = blockIdx.x * SW_WAVES + wv;
    return {&s_d, &s_E, lds_all[wv], g < d_arg.n_slots ? g : -1, (int)(threadIdx.x & 63)};
}
// Up to `sims` simulations of the wave's slot; the last leaf stays pending.  Returns whether one is (wave-uniform).
__device__ __forceinline__ bool dc_swr_sims(const DCRolloutWave &w, int sims) {
    bool pending = false; // (no leaf is pending on entry, or the first tree step applies it: see dc_search_wave_body)
    for (int s = 0; s < sims; s++) {
        pending = dc_swr_tree(*w.d, *w.E, w.g, w.lane, w.tl) >= 0;
        if (!pending) break; // (uniform) no game or no simulations left: every further step is a no-op (see the head of this file)
        dc_swr_rollout(*w.d, w.g, w.lane);
    }
    return pending;
}
__global__ void __launch_bounds__(64 * SW_WAVES) k_dc_search_wave_rollout(TreeDev d_arg, DCEdges E_arg, int sims) {
    const DCRolloutWave w = dc_swr_prologue(d_arg, E_arg);
    if (w.g < 0) return;
    if (dc_swr_sims(w, sims)) dc_swr_apply(*w.d, *w.E, w.g, w.lane, w.tl); // the last simulation's evaluation
}
