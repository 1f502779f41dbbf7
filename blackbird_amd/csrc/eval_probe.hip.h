// eval_probe.hip.h -- the evaluation cache (net.hip.h EvalCache) for the asynchronous-round launch structure.
//
// A round is k_tree_async appending the leaves that need the network to a compacted list (post_count / post_slot), then the
// network launches over that list; their time is proportional to the list's length.  k_eval_cache_probe runs in between, on
// the same stream: one wave per posted leaf looks its position up in the table.
//   hit:  the leaf is finished here -- value from the entry, dense_prior_tail on the cached priors with the slot's own
//         (game id, serial), i.e. the node's prior noise drawn exactly as head_one draws it -- and taken back out of
//         d.evals[slot], which keeps counting tower runs (mega2.hip.h does the same);
//   miss: the slot goes on a second compacted list (miss_count / miss_slot), which is what the network launches take; their
//         heads store the entry (head_one's cache_entry; the key is formed from the leaf state again there) into the way of
//         the bucket that the probe chose from the keys it read (miss_way[slot]: eval_cache_pick_way).
// A board without a key (G::cache_key == 0) is a miss that is neither probed nor stored.  The table rules are those of
// net.hip.h: 16-byte single-lane accesses, every chunk carries its own key, no fences, key 0 never probed or stored.
// Nothing depends on two leaves of a round being different positions: two hits of a key read the same entry, two misses
// both run the tower and store the same bits into the same way (duplicates inside a round are not merged), and a probe that
// reads an entry while another view's head stores it sees either all four chunks of its key or a miss.
#pragma once
#include "net.hip.h"

// grid: ceil(n_slots / 4) workgroups of 4 waves, wave w of workgroup b <-> list entry 4 b + w (waves past *n_ptr idle).
// miss_count: the view's [4] counters, rotated like post_count -- this round appends to [round & 3] and clears
// [(round + 2) & 3] for the round after next (the launches of one view are ordered by its stream).
template <class G>
__global__ void __launch_bounds__(256)
k_eval_cache_probe(NetDev nd, EvalCache cache, const int *n_ptr, const int *slot_list, int *miss_count, int round, int *miss_slot,
                   unsigned char *miss_way,
                   const typename G::State *states, const uint32_t *game_id, const int32_t *serial, int noise, float *value_out,
                   float *policy_out, int pstride, uint64_t *evals, unsigned long long *ctr) {
    static_assert(G::CACHE_KEY, "a game whose positions have a one-word key (Connect4)");
    __shared__ int s_slot[4], s_probe[4], s_base; // per wave: slot to append (-1: none), 1 + hit when probed (0: not)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63; // (scalar: list entry, slot, board and key are)
    const int n = *n_ptr, pos = blockIdx.x * 4 + wave;
    const bool live = pos < n;
    // clamped addresses, selected afterwards: no load sits in a divergent branch (entry 0 of a list that was zeroed at
    // allocation is a slot number, key 0 maps to the table's bucket 0); what depends on `live` alone is a uniform branch
    const int slot = slot_list[live ? pos : 0];
    const typename G::State st = states[slot];
    const uint64_t key = live ? G::cache_key(st) : 0; // (wave-uniform)
    u32x4 *const bucket = eval_cache_bucket(cache, key);
    const u32x4 chunk = eval_cache_load(bucket, lane); // issued before anything that does not depend on it
    if (blockIdx.x == 0 && threadIdx.x == 0) miss_count[(round + 2) & 3] = 0;
    float cv = 0.f, cpr = 0.f;
    int way = 0;
    const bool hit = eval_cache_hit<G>(chunk, key, lane, cv, cpr, way) && key != 0; // (an empty entry carries key 0)
    if (hit) {
        if (lane == 0) {
            value_out[slot] = cv;
            evals[slot] -= 1;
        }
        dense_prior_tail<G>(nd, cpr, slot, true, game_id, serial, noise, policy_out, pstride, lane);
    }
    if (lane == 0) {
        s_slot[wave] = live && !hit ? slot : -1;
        if (live && !hit) miss_way[slot] = (unsigned char)way;
        s_probe[wave] = key ? 1 + (int)hit : 0;
    }
    __syncthreads();
    // one append and one pair of counter updates per workgroup
    if (threadIdx.x == 0) {
        int n_miss = 0, n_probe = 0, n_hit = 0;
        for (int w = 0; w < 4; w++) {
            n_miss += s_slot[w] >= 0;
            n_probe += s_probe[w] > 0;
            n_hit += s_probe[w] > 1;
        }
        s_base = n_miss ? atomicAdd(&miss_count[round & 3], n_miss) : 0;
        if (n_probe && ctr) {
            if (n_hit) atomicAdd(&ctr[0], (unsigned long long)n_hit);
            atomicAdd(&ctr[1], (unsigned long long)n_probe);
        }
    }
    __syncthreads();
    if (lane == 0 && s_slot[wave] >= 0) {
        int rank = 0;
        for (int w = 0; w < wave; w++) rank += s_slot[w] >= 0;
        miss_slot[s_base + rank] = slot;
    }
}
