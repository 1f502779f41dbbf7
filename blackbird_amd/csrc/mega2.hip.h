// mega2.hip.h -- persistent self-play kernel: tree search and network evaluation of the SAME 16 games share one
// workgroup (one CU) and hand leaves / evaluations to each other through that CU's LDS alone.
//
// With one launch per phase (k_tree_async, k_net_compact) every round waits for the deepest descent among all 4096
// games and the MFMA units idle while the latency-bound tree kernel runs.  Here the 16 games of a workgroup circulate
// freely between
//     4 tree waves   (4 games each, S lanes per game): apply result -> [move] -> descend -> post leaf
//     8 network waves (2 per SIMD, one position each): pop leaf -> tower + heads -> publish result
// through an LDS ring of game indices and a per-game state word.  A network wave's head/softmax VALU work
// overlaps its SIMD partner's MFMAs (the partners drift apart by themselves), and nobody waits for the
// slowest game of a set.
//
// Synchronisation is workgroup-scope only (LDS atomics + __threadfence_block, all waves on one CU share L1),
// so it is placement-independent.  Every wait loop is bounded by wall-clock time: a protocol bug ends the
// launch with the abort word set (reported through the overflow counter) instead of hanging the GPU.
#pragma once
#include "net.hip.h"
#include "net_x3.hip.h"
#include "tree.hip.h"

#define MEGA_RMAX 4          // residual blocks whose weights fit the 160 KiB LDS next to the activations
// packed head parameters that fit next to them.  Every array of NetDev::head is padded to 4 floats (bb_load_weights), so a 16-filter
// network packs 88 + 3 * pad4(D) floats for Connect4 and 96 + 3 * pad4(D) for TicTacToe: 136 / 144 at the default D = 16, and
// D <= 32 fits (Connect4 184; TicTacToe exactly 192 at D = 29 .. 32).  D >= 33 plays as rounds (host_selfplay.hip.h selfplay_structure).
#define MEGA_HEAD_FLOATS 192

// Waves of the workgroup = NETW network waves + the tree waves.  float32-MFMA network: 12 waves (8 + 4) at 168 VGPRs;
// bf16-pipe network (X3): 12 waves (8 + 4) at 168 VGPRs for Connect4, 8 waves (4 + 4) for TicTacToe (4 games of 16 lanes per
// tree wave).
#define MEGA2_QCAP 32
#ifndef BB_TREE_IDLE_SLEEP
#define BB_TREE_IDLE_SLEEP 4 // s_sleep argument (x 64 cycles) of a tree wave that finds none of its games ready
#endif
#ifndef BB_NET_IDLE_SLEEP
#define BB_NET_IDLE_SLEEP 4  // ... of a network wave that finds the queue empty
#endif

__device__ __forceinline__ int lds_load(volatile int *p) { return *p; }
// Release for a flag that lives in LDS while the data lives in global memory: the workgroup-scope fence
// the compiler emits waits for LDS traffic only, so a flag store could pass this wave's global stores.
__device__ __forceinline__ void release_global_then_lds() {
    __threadfence_block();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}


// ---- per-game control state shadowed in LDS for the lifetime of the launch ----------------------------------
// async_game touches a dozen per-slot scalars, the evaluator mailbox and the recorded path of a game on every
// call, each a dependent L2 round trip.  The persistent kernel owns its 16 games for the whole launch, so it
// copies that state into LDS once, points a private TreeDev at the copies and writes everything back before the
// launch ends.  The tree code indexes these arrays with the workgroup-LOCAL game number (TreeDev::pool_g0 carries the
// workgroup's first slot for the node pools, which stay in HBM), so the pointers are the plain addresses of __shared__
// arrays: the compiler sees the LDS address space and emits ds_read / ds_write with immediate offsets from one base
// register, instead of flat_* instructions through twenty 64-bit generic addresses held in VGPR pairs.
// The rows it keeps (B: always, R: in its REC form), and the order it copies them in, by name alone.  That is not the rows' order:
// the register allocation of the whole kernel follows the order of the copy loops.  A name that is no member does not compile,
// and the two lists' lengths are compared (which one name twice and another left out would still pass).
#define BB_QUEUE_SHADOWED(B, R) BB_SLOTS_TREE(B, B, R) BB_SLOTS_MAILBOX(B, B) BB_SLOTS_RESUME(B)
#define BB_QUEUE_COPY_ORDER(X)                                                                                           \
    X(root) X(root_N) X(n_nodes) X(ply) X(sims_left) X(pend_leaf) X(pend_expand) X(path_len) X(game_lid) X(sim_serial)   \
    X(leaf_serial) X(resume_cur) X(resume_depth) X(leaf_game_id) X(root_W) X(eval_value) X(eval_policy) X(evals) X(ctr)  \
    X(path) X(root_pp) X(leaf_flags)
#define BB_QUEUE_COPY_ORDER_REC(X) X(path_N) X(path_all) X(path_W)
#define BB_COUNT(...) +1
#define BB_SHADOW_PER(f) ((int)(sizeof(f) / sizeof(f[0])) / GW) // its row's `per`
template <class G, int GW, bool REC>
struct GameShadow {
    static constexpr int S = G::S, MP = G::MAXPATH, PS = S;
#define X(T, f, per) T f[REC ? GW * (per) : 1];
    BB_QUEUE_SHADOWED(BB_SHADOW_MEMBER, X)
#undef X
    typename G::State leaf_state[GW];
    static_assert(0 BB_QUEUE_COPY_ORDER(BB_COUNT) BB_QUEUE_COPY_ORDER_REC(BB_COUNT) == 0 BB_QUEUE_SHADOWED(BB_COUNT, BB_COUNT), "a row is not copied");
    // all threads of the workgroup; n = games of this workgroup that exist (g0 + i < n_slots)
    __device__ __forceinline__ void load(const TreeDev &d, int g0, int n, int nthreads) {
#define X(f) BB_SHADOW_LOAD(d, f, BB_SHADOW_PER(f))
        BB_QUEUE_COPY_ORDER(X)
        if constexpr (REC) { BB_QUEUE_COPY_ORDER_REC(X) }
#undef X
        for (int i = threadIdx.x; i < n; i += nthreads) leaf_state[i] = ((const typename G::State *)d.leaf_state)[g0 + i];
    }
    __device__ __forceinline__ void store(const TreeDev &d, int g0, int n, int nthreads) {
#define X(f) BB_SHADOW_STORE(d, f, BB_SHADOW_PER(f))
        BB_QUEUE_COPY_ORDER(X)
        if constexpr (REC) { BB_QUEUE_COPY_ORDER_REC(X) }
#undef X
        for (int i = threadIdx.x; i < n; i += nthreads) ((typename G::State *)d.leaf_state)[g0 + i] = leaf_state[i];
    }
    __device__ __forceinline__ TreeDev local(const TreeDev &d, int g0) {
        TreeDev r = d;
#define X(f) r.f = f;
        BB_QUEUE_COPY_ORDER(X)
        if constexpr (REC) { BB_QUEUE_COPY_ORDER_REC(X) }
#undef X
        r.leaf_state = leaf_state;
        r.pool_g0 = g0;
        return r;
    }
};

struct QueueCtl {
    int q[MEGA2_QCAP];
    int head, tail, tree_done, abort_flag;
};

// Pop one queued game for a network wave: >= 0 game index, -1 nothing queued right now, -2 finished (or aborted).
// Deliberately NOT inlined: with the lane-0 pop inlined into the wave's loop the compiler threads the other 63
// lanes past it, and the wave then runs the network with lane 0 split off from the rest.
__device__ __attribute__((noinline)) int queue_pop(QueueCtl *c, long long t_start, long long t_limit, int n_tree) {
    int li = -1;
    if ((threadIdx.x & 63) == 0) {
        int h = lds_load(&c->head), t = lds_load(&c->tail);
        if (h < t) {
            if (atomicCAS(&c->head, h, h + 1) == h) { // compare-and-swap so that an empty queue is never over-popped
                volatile int *slot = &c->q[h & (MEGA2_QCAP - 1)];
                for (int spin = 0; spin < (1 << 20) && (li = *slot) < 0; spin++) __builtin_amdgcn_s_sleep(1);
                *slot = -1; // at most 16 entries are ever outstanding, so the slot is not reused before this
                if (li < 0) {
                    c->abort_flag = 1;
                    li = -2;
                }
            }
        } else if (lds_load(&c->tree_done) >= n_tree) {
            li = -2;
        } else if (wall_clock64() - t_start > t_limit || lds_load(&c->abort_flag)) {
            c->abort_flag = 1;
            li = -2;
        }
    }
    return __builtin_amdgcn_readfirstlane(li);
}

// Tree-wave side: publish this call's outcome for every game leader lane (`leader`) of the wave.  Not inlined for the
// same reason as queue_pop: the lanes of the wave must come back from here together.
// GLOBAL_TOO: the consumer of the queue entry also reads what this wave wrote to global memory (the network wave applies
// the result to the tree itself: float32 form); otherwise only the mailbox in LDS has to be visible.
template <bool GLOBAL_TOO>
__device__ __attribute__((noinline)) void queue_push(QueueCtl *c, uint8_t *state_byte, bool leader, bool posted, int li) {
    if (GLOBAL_TOO) release_global_then_lds(); // mailbox + tree writes before the queue entry
    else __threadfence_block();
    if (leader) {
        if (posted) {
            *(volatile uint8_t *)state_byte = 1;
            int idx = atomicAdd(&c->tail, 1); // the entry becomes valid when its slot turns non-negative
            *(volatile int *)&c->q[idx & (MEGA2_QCAP - 1)] = li;
        } else {
            *(volatile uint8_t *)state_byte = 0;
        }
    }
}

// X3: the network runs on the bf16 matrix pipe (net_x3.hip.h): its packed operands are 1.5x the float32 ones, but it needs
// far fewer matrix cycles per evaluation.
template <class G, int NETW, bool X3 = false, int WAVES = 12>
__global__ void __launch_bounds__(WAVES * 64) k_selfplay_queue(TreeDev dg, NetDev nd, NetX3 x3, int noise_on, int limit_s, int own_visits) {
    constexpr int MEGA2_THREADS = WAVES * 64;
    // The wave that holds an evaluation also expands the leaf and backs the value up when the tree waves are the busier side
    // (float32 network: they share their SIMD's vector ALUs with the f32 MFMAs); beside the bf16-pipe network the network
    // waves are the busy side and the tree waves take the result back.
    constexpr bool NET_APPLIES = !X3;
    constexpr int S = G::S, GW = 16, TREEW = WAVES - NETW, GPT = (GW + TREEW - 1) / TREEW; // games per workgroup, tree waves, games per tree wave
    static_assert(GPT * S <= 64, "a tree wave holds at most 64 / S games");
    using NG = NetGeom<G, 1>;
    constexpr int RMAX = MEGA_RMAX, STEPS0 = NG::STEPS0;
    using XG = X3Geom<G>;
    constexpr int EPI_F = (1 + 2 * RMAX) * 48, HEAD_F = MEGA_HEAD_FLOATS;
    // operand floats: float32 form [wt][w0], x3 form [w0 bytes][wt bytes]; then epilogue constants and head parameters
    constexpr int WT_F = X3 ? 2 * RMAX * XG::LAYER12_B / 4 : 2 * RMAX * 9 * 64 * 4, W0_F = X3 ? XG::W0_B / 4 : STEPS0 * 64;
    constexpr int WAVE_F = X3 ? XG::WAVE_BYTES / 4 : NG::WAVE_FLOATS;
    __shared__ __attribute__((aligned(16))) float lds[NETW * WAVE_F];
    constexpr int WH_F = X3 ? 3 * 64 * 16 / 4 : 0; // (x3: the head convolutions' three MFMA operands)
    __shared__ __attribute__((aligned(16))) float wlds[WT_F + W0_F + EPI_F + HEAD_F + WH_F];
    __shared__ QueueCtl qc;
    __shared__ GameShadow<G, GW, X3> shadow;
    // Per-game state: 0 owned by its tree wave, 1 leaf queued / being evaluated, 2 result published.  One byte per game, the
    // games of a tree wave next to each other (GSI): the wave sees all of its games' states in ONE 8-byte LDS read.
    static_assert(GPT <= 8, "a tree wave's game states are one 8-byte word");
    __shared__ __attribute__((aligned(8))) uint8_t gstate[TREEW * 8];
#define GSI(li) ((((li) % TREEW) << 3) + (li) / TREEW)
    __shared__ int myslot[NETW];
    // Visits are not dealt per game.  A workgroup starts with its own share (`own_visits` per slot: 7/8 of the launch's visits,
    // so that every slot advances even when more workgroups are launched than the chip holds at once -- the resident ones
    // cannot drain what belongs to the later ones) and every game of the workgroup searches until that is used up; the last
    // eighth is ONE launch-wide pool (dg.visit_pool) that the workgroups then draw from in chunks until it is dry.  With a
    // fixed count per game the pipeline of a workgroup ran empty game by game at the end of every launch and the launch
    // waited for its slowest workgroup (~35 ms of a 16-step launch); a game's results do not depend on when its visits happen.
    __shared__ int wg_pool, wg_dry, wg_refill;
    constexpr int CHUNK = GW * 32;
    IF_STAMPS(__shared__ long long ts_post[GW], ts_done[GW];) // wall clock: leaf posted, result published
    const int wave = threadIdx.x >> 6, l64 = threadIdx.x & 63;
    const int g0 = blockIdx.x * GW;
    const int n_mine = dg.n_slots - g0 < GW ? dg.n_slots - g0 : GW;
    shadow.load(dg, g0, n_mine, MEGA2_THREADS);
    const TreeDev d = shadow.local(dg, g0); // everything below works on the LDS copies, indexed by the local game number
    if (threadIdx.x == 0) {
        qc.head = 0;
        qc.tail = 0;
        qc.tree_done = 0;
        qc.abort_flag = 0;
        wg_pool = n_mine * own_visits;
        wg_dry = 0;
        wg_refill = 0;
    }
    if (threadIdx.x < TREEW * 8) gstate[threadIdx.x] = 0;
    net_stamps_zero();
    if (threadIdx.x < MEGA2_QCAP) qc.q[threadIdx.x] = -1;
    for (int i = threadIdx.x; i < NETW * WAVE_F; i += MEGA2_THREADS) lds[i] = 0.f;
    NetDev ndl = nd;
    NetX3 x3l = x3;
    {
        const float *gwt = X3 ? (const float *)x3.wt12 : (const float *)nd.wt;
        const float *gw0 = X3 ? (const float *)x3.w0 : nd.w0;
        const int wt_used = X3 ? 2 * nd.R * XG::LAYER12_B / 4 : 2 * nd.R * 9 * 64 * 4;
        for (int i = threadIdx.x; i < wt_used; i += MEGA2_THREADS) wlds[i] = gwt[i];
        for (int i = threadIdx.x; i < W0_F; i += MEGA2_THREADS) wlds[WT_F + i] = gw0[i];
        x3l.wt12 = (const unsigned char *)wlds; // (x3l.wt3 stays in global memory)
        x3l.w0 = (const unsigned char *)(wlds + WT_F);
        for (int i = threadIdx.x; i < (1 + 2 * nd.R) * 48; i += MEGA2_THREADS) wlds[WT_F + W0_F + i] = nd.epi[i];
        for (int i = threadIdx.x; i < nd.head_floats; i += MEGA2_THREADS) wlds[WT_F + W0_F + EPI_F + i] = nd.head[i];
        if constexpr (X3) {
            for (int i = threadIdx.x; i < WH_F; i += MEGA2_THREADS) wlds[WT_F + W0_F + EPI_F + HEAD_F + i] = ((const float *)x3.wh)[i];
            x3l.wh = (const unsigned char *)(wlds + WT_F + W0_F + EPI_F + HEAD_F);
        }
        ndl.wt = (const f32x4 *)wlds;
        ndl.w0 = wlds + WT_F;
        ndl.epi = wlds + WT_F + W0_F;
        ndl.head = wlds + WT_F + W0_F + EPI_F;
    }
    __syncthreads();
    const long long t_start = wall_clock64();
    const long long t_limit = 100000000ll * limit_s; // wall clock runs at 100 MHz

    if (wave >= NETW) { // ---------------- tree waves ----------------
        const int tw = wave - NETW;
        // the tree waves are the latency chain of every game: let them win issue arbitration against the
        // throughput-bound network waves of their SIMD (+8 % games/s)
        __builtin_amdgcn_s_setprio(3);
        const int li = (l64 / S) * TREEW + tw, lane = l64 % S; // games are dealt round-robin to the tree waves
        const bool mine = l64 < GPT * S && li < GW && g0 + li < d.n_slots;
        const int g = li; // local game number: index of the LDS copies
        bool alive = mine && d.game_lid[mine ? g : 0] >= 0; // false once the slot has run out of games (or never had one)
        IF_STAMPS(long long t_work = 0, t_all0 = clock64(), n_calls = 0, n_lanes = 0, t_pick = 0, n_pick = 0;)
        // A leaf goes to the network waves the moment its mailbox is written (async_game's on_post hook), not when the call
        // returns: a call of this wave lasts as long as the slowest of its games' descents.  The network wave that evaluates the
        // leaf also draws its prior noise (head_one).
        auto early_post = [&](int gg, int ln) __attribute__((always_inline)) {
            if (NET_APPLIES) release_global_then_lds(); // mailbox (+ tree writes) before the queue entry
            else __threadfence_block();
            if (ln == 0) {
                IF_STAMPS(ts_post[li] = wall_clock64();)
                *(volatile uint8_t *)&gstate[GSI(li)] = 1;
                const int idx = atomicAdd(&qc.tail, 1); // the entry becomes valid when its slot turns non-negative
                *(volatile int *)&qc.q[idx & (MEGA2_QCAP - 1)] = li;
            }
        };
        for (;;) {
            int stt = mine ? (int)*(volatile uint8_t *)&gstate[GSI(li)] : 1;
            const int pool = lds_load(&wg_pool), dry = lds_load(&wg_dry);
            if (pool < CHUNK / 4 && !dry && __any(alive)) { // (wave-uniform) top the workgroup's share up before it runs out
                if (l64 == 0 && atomicCAS(&wg_refill, 0, 1) == 0) {
                    int old = atomicSub(d.visit_pool, CHUNK);
                    int got = old < 0 ? 0 : old < CHUNK ? old : CHUNK;
                    if (got) atomicAdd(&wg_pool, got);
                    else *(volatile int *)&wg_dry = 1;
                    __threadfence_block();
                    *(volatile int *)&wg_refill = 0;
                }
                if (pool <= 0) { // another wave's refill is on its way: wait for it like every other wait, bounded by wall-clock time
                    __builtin_amdgcn_s_sleep(1);
                    int late = wall_clock64() - t_start > t_limit || lds_load(&qc.abort_flag);
                    if (__builtin_amdgcn_readfirstlane(late)) {
                        qc.abort_flag = 1;
                        break;
                    }
                    continue;
                }
            }
            bool ready = mine && alive && pool > 0 && stt != 1;
            bool busy = mine && ((alive && pool > 0) || (alive && !dry) || stt == 1); // visits left to draw, or a leaf of mine is in flight
            if (!__any(busy)) break;
            if (__any(ready)) {
                __threadfence_block(); // acquire: the network wave's results for state 2
                bool posted = false;
                IF_STAMPS(long long ts = clock64(); n_calls++; n_lanes += __popcll(__ballot(ready)) / S;)
                IF_STAMPS(if (ready && lane == 0 && stt == 2) { t_pick += wall_clock64() - ts_done[li]; n_pick++; })
                LevelStamps light;
                if (ready) {
                    posted = async_game<G, X3>(d, g, lane, early_post, &light);
                    if (d.game_lid[g] < 0) alive = false; // slot ran out of games
                }
                level_stamps_flush(d.stamps, light, ready && lane == 0, l64);
                {
                    int used = __popcll(__ballot(ready && lane == 0));
                    if (l64 == 0) atomicSub(&wg_pool, used);
                }
                // (posted leaves went to the network waves inside the call: early_post; the others go back to their tree wave)
                queue_push<NET_APPLIES>(&qc, &gstate[GSI(li < GW ? li : 0)], ready && lane == 0 && !posted, false, li);
                IF_STAMPS(t_work += clock64() - ts;)
            } else {
                __builtin_amdgcn_s_sleep(BB_TREE_IDLE_SLEEP);
                int late = wall_clock64() - t_start > t_limit || lds_load(&qc.abort_flag);
                if (__builtin_amdgcn_readfirstlane(late)) {
                    qc.abort_flag = 1;
                    break;
                }
            }
        }
        if (l64 == 0) atomicAdd(&qc.tree_done, 1);
        IF_STAMPS(if (l64 == 0) stamp_add_all(d.stamps, QS_TREE_WORK, t_work, QS_TREE_ALIVE, clock64() - t_all0, QS_TREE_WAVES, 1, QS_TREE_CALLS, n_calls, QS_TREE_GAMES, n_lanes);)
        IF_STAMPS(if (lane == 0 && n_pick) stamp_add_all(d.stamps, QS_PICK_WAIT, t_pick, QS_PICKS, n_pick);)
    } else { // ---------------- network waves ----------------
        float *wl = lds + wave * WAVE_F;
        // The evaluation cache (net.hip.h; off when dg.eval_cache is null): a hit costs the prior-noise tail instead of the tower.
        // d.evals keeps counting tower runs -- the tree wave counted the leaf when it posted it, so a hit takes it back.
        constexpr bool CACHE = X3 && G::CACHE_KEY;
        const EvalCache ecache = {(u32x4 *)dg.eval_cache, dg.eval_cache_log2};
        unsigned long long n_probes = 0, n_hits = 0;
        IF_STAMPS(long long t_work = 0, t_all0 = clock64(), n_evals = 0, t_qwait = 0;)
        for (;;) {
            const int li = __builtin_amdgcn_readfirstlane(queue_pop(&qc, t_start, t_limit, TREEW)); // scalar: uniform branches below
            if (li == -2) break;
            if (li < 0) {
                __builtin_amdgcn_s_sleep(BB_NET_IDLE_SLEEP);
                continue;
            }
            __threadfence_block(); // acquire: the tree wave's mailbox writes
            IF_STAMPS(long long ts = clock64(); n_evals++; t_qwait += wall_clock64() - ts_post[li];)
            if (l64 == 0) myslot[wave] = li;
            if constexpr (X3) {
                int probe = -1;
                net_body_x3<G, true, false, CACHE>(ndl, x3l, 1, 0, &myslot[wave], (unsigned char *)wl, (const typename G::State *)d.leaf_state, nullptr,
                                     d.leaf_game_id, d.leaf_serial, noise_on, d.eval_value, nullptr, d.eval_policy, S, false, nullptr,
                                     ecache, &probe);
                if constexpr (CACHE) {
                    n_probes += probe >= 0;
                    if (probe > 0) {
                        n_hits++;
                        if (l64 == 0) d.evals[li] -= 1;
                    }
                }
            } else
                net_body<G, 1, 2>(ndl, 1, 0, &myslot[wave], wl, (const typename G::State *)d.leaf_state, nullptr,
                                  d.leaf_game_id, d.leaf_serial, noise_on, d.eval_value, nullptr, d.eval_policy, S, false);
            if constexpr (NET_APPLIES) {
            // The evaluated leaf is expanded and its value backed up right here, by the wave that holds the result, instead
            // of waiting until the game's tree wave comes round (the tree waves are every game's latency chain and the
            // busier side of the queue: 91 % against 67 %; a result used to wait ~10 us to be picked up).  Same function,
            // same lane layout (lane i <-> child slot i on lanes 0..S-1), so the same bits.
            __threadfence_block(); // the mailbox writes of net_body (other lanes) before phase_apply reads them
            IF_STAMPS_NET(NetStamps na;)
            if (l64 < S) {
                phase_apply<G>(d, li, l64);
                if (l64 == 0) d.sims_left[li] -= 1;
            }
            IF_STAMPS_NET(na.stop(NS_APPLY, l64);)
            }
            release_global_then_lds(); // value / policy (and the tree rows) before the state word
            IF_STAMPS(if (l64 == 0) ts_done[li] = wall_clock64();)
            if (l64 == 0) *(volatile uint8_t *)&gstate[GSI(li)] = 2;
            IF_STAMPS(t_work += clock64() - ts;)
        }
        IF_STAMPS(if (l64 == 0) stamp_add_all(d.stamps, QS_NET_WORK, t_work, QS_NET_ALIVE, clock64() - t_all0, QS_NET_WAVES, 1, QS_EVALS, n_evals, QS_QUEUE_WAIT, t_qwait);)
        if (CACHE && l64 == 0 && n_probes && dg.eval_cache_ctr) {
            atomicAdd(&dg.eval_cache_ctr[0], n_hits);
            atomicAdd(&dg.eval_cache_ctr[1], n_probes);
        }
    }
    __syncthreads();
    net_stamps_flush();
    if (qc.abort_flag) { // a wait ran into the wall-clock limit: surfaces as bb_counters.overflow
        if (threadIdx.x == 0) d.ctr[6] += 1;
        // a leaf that was queued but never evaluated must not be applied by the next launch (its mailbox holds the
        // previous evaluation): drop it, the simulation is redone from the root
        if ((int)threadIdx.x < n_mine && gstate[GSI(threadIdx.x)] == 1) shadow.pend_leaf[threadIdx.x] = -1;
    }
    __syncthreads();
    shadow.store(dg, g0, n_mine, MEGA2_THREADS); // hand the per-game state back to HBM
}
