// stamps.hip.h -- the kernels' diagnostics: in-kernel cycle stamps and the network's ablation switches.
//
// Five compile-time switches, all off in the product build, where everything in this header is an empty struct, a function
// with an empty body, a constant 0 or a macro without expansion: the product build's device code does not contain an
// instruction of it.  This header holds the only #if on the switches in the device headers; the kernels themselves are free
// of preprocessor conditionals.  A diagnostic build is the Makefile's command with the switches added and another output
// name, from the repository root:
//
//   hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off <switches> -shared -o tools/<lib> blackbird_amd/csrc/engine.hip
//
// BB_STAMPS           shader-clock (clock64) and wall-clock (wall_clock64, 100 MHz) stamps of the tree kernels, the two
//                     persistent self-play kernels and the DragonChess phases, summed into TreeDev::stamps (the word map
//                     below); read and cleared by bb_debug_stamps, bb_debug_host_stamps maps the buffer to the host.
//                     Read by tools/tree_stamps.py, queue_stamps.py, mega_stamps.py, dc_stamps.py, dc_pair_where.py.
//                     Switches: -DBB_STAMPS, as tools/libbb_stamps.so.
// BB_STAMPS_LIGHT     (with BB_STAMPS) async_game times its own descent loops per tree level: LevelStamps.  Words 6, 7, 11
//                     and 12 then carry these figures.  Read by tools/tree_light.py (and queue_stamps.py with LIGHT=1).
//                     Switches: -DBB_STAMPS -DBB_STAMPS_LIGHT, as tools/libbb_stamps_deep.so.
// BB_STAMPS_NET       (with BB_STAMPS) cycles per section of net_body / net_body_x3 inside the persistent kernels, summed
//                     per workgroup in LDS (s_net_stamps) and flushed to g_net_stamps; read and cleared by bb_debug_net_stamps.
//                     Read by tools/dc_net_stamps.py and queue_stamps.py with NETSTAMPS=1.
//                     Switches: -DBB_STAMPS -DBB_STAMPS_NET, as tools/libbb_stamps_net.so.
// BB_STAMPS_NET_SUB   (with BB_STAMPS_NET) splits net_body_x3's prologue into sections 5..7 (NetStamps::sub); section 0 is
//                     then the rest of the prologue.  Same tools and library name as BB_STAMPS_NET.
// BB_DIAG             the ablation argument of bb_timing_net: NetDev::dbg switches parts of the network off (ND_DBG; the
//                     results are wrong when a bit is set).  Read by tools/net_ablate.py, dc_net_ablate.py.
//                     Switches: -DBB_DIAG.
//
// ---- the stamp-word map --------------------------------------------------------------------------------------------------
// TreeDev::stamps is STAMP_COPIES copies of STAMP_WORDS words; bb_debug_stamps sums the copies.  The Connect4 kernels add to
// copy 0 with atomics when a wave ends; the DragonChess kernels collect in their wave's LDS scratch (dst_add: atomics inside
// the timed sections would sit in front of every later s_waitcnt) and flush once, game g to copy g & 63 (dst_flush).
// The families share the buffer and overlap in the numbers: a tool reads the words of the kernels its run launched.
// "ticks" are shader clocks unless the entry says wall clock.
//
//  word | k_tree_step /        | k_tree_async, tree waves:  | k_selfplay_queue (mega2.hip.h)     | DragonChess: k_dc_tree_step,
//       | phase_select         | BB_STAMPS_LIGHT            |                                    | k_dc_selfplay_fused (DST_*)
//  -----+----------------------+----------------------------+------------------------------------+-------------------------------
//    0  | apply ticks          |                            | net waves: ticks at work           | apply ticks (fused: apply + select)
//    1  | fence ticks          |                            | net waves: ticks alive             | select: tree levels
//    2  | select ticks         |                            | tree waves: ticks at work          | select ticks (fused: network)
//    3  |                      |                            | tree waves: ticks alive            | apply: second round of loads
//    4  | wave-steps counted   |                            | net waves counted                  | game-steps counted
//    5  | select: row-load     |                            | tree waves counted                 | expand: gather + noise
//       | ticks                |                            |                                    |
//    6  | select: loop         | longest game of the call:  | (LIGHT column)                     | expand: dc_np_sum
//       | iterations           | ticks in its descent loops |                                    |
//    7  | select: descents     | ... its tree levels        | (LIGHT column)                     | expand: edge rows written
//    8  |                      |                            | result pick-up wait (wall clock)   | expansions with priors counted
//    9  |                      |                            | results picked up                  | expand: move generation
//   10  |                      |                            | queue wait of a leaf (wall clock)  | apply: entry -> first loads complete
//   11  |                      | ... its row-load wait      | (LIGHT column)                     | select: first loads
//   12  |                      | ... its PUCT + argmax      | (LIGHT column)                     | select: node rows
//   13  |                      |                            | tree waves: async_game call rounds | select: edge rows
//   14  |                      |                            | tree waves: games in those rounds  | select: PUCT + argmax
//   15  |                      |                            | net waves: evaluations             | select: child creation, leaf, tail
//
// g_net_stamps / s_net_stamps (BB_STAMPS_NET), NET_STAMP_WORDS words, cycles summed over the network waves' calls:
//    0 prologue (BB_STAMPS_NET_SUB: what 5..7 leave of it)   1 first conv   2 tower   3 1x1 head convs   4 head tail
//    5 k_selfplay_queue, float32 network: expand + backup on the network wave (phase_apply)
//      BB_STAMPS_NET_SUB, net_body_x3: loads issued + zero fill        6 (SUB) state to LDS        7 (SUB) planes
#pragma once
#include <cstdint>

constexpr int STAMP_WORDS = 16, STAMP_COPIES = 64;            // TreeDev::stamps
constexpr int STAMP_BUFFER_WORDS = STAMP_WORDS * STAMP_COPIES;
constexpr int STAMP_BUFFER_BYTES = STAMP_BUFFER_WORDS * 8;
constexpr int NET_STAMP_WORDS = 8;                            // g_net_stamps

// the words one kernel family owns by name (the numbers are what the tools index by: they do not change)
enum { // k_tree_step / phase_select
    TS_APPLY = 0, TS_FENCE = 1, TS_SELECT = 2, TS_WAVES = 4, TS_ROW_LOAD = 5, TS_ITERATIONS = 6, TS_DESCENTS = 7
};
enum { // async_game's LevelStamps, from k_tree_async and the tree waves of k_selfplay_queue
    LS_LOOP = 6, LS_LEVELS = 7, LS_ROW_LOAD = 11, LS_PUCT = 12
};
enum { // k_selfplay_queue
    QS_NET_WORK = 0, QS_NET_ALIVE = 1, QS_TREE_WORK = 2, QS_TREE_ALIVE = 3, QS_NET_WAVES = 4, QS_TREE_WAVES = 5,
    QS_PICK_WAIT = 8, QS_PICKS = 9, QS_QUEUE_WAIT = 10, QS_TREE_CALLS = 13, QS_TREE_GAMES = 14, QS_EVALS = 15
};
enum { // the DragonChess phases (dst_add)
    DST_APPLY = 0, DST_LEVELS = 1, DST_SELECT = 2, DST_APPLY_LOADS2 = 3, DST_STEPS = 4, DST_EXP_GATHER = 5, DST_EXP_SUM = 6,
    DST_EXP_EDGES = 7, DST_EXPANSIONS = 8, DST_EXP_MOVEGEN = 9, DST_APPLY_LOADS1 = 10, DST_SEL_FIRST = 11, DST_SEL_NODE = 12,
    DST_SEL_EDGE = 13, DST_SEL_PUCT = 14, DST_SEL_REST = 15
};
enum { // net_body / net_body_x3 sections
    NS_PROLOGUE = 0, NS_CONV0 = 1, NS_TOWER = 2, NS_HEAD_CONVS = 3, NS_HEAD_TAIL = 4, NS_APPLY = 5, NS_SUB_LOADS = 5,
    NS_SUB_STATE = 6, NS_SUB_PLANES = 7
};

// The DragonChess stamp words live in the wave's LDS scratch, DST words past the policy image, its 112 floats of sum scratch
// AND the network's activations, which share the scratch in mega_dc.hip.h (tree_dc.hip.h sizes the scratch: DC_LDS_FLOATS).
constexpr int DC_STAMP_OFF = 5136;

// ---- the vocabulary ------------------------------------------------------------------------------------------------------
// Two kinds.  Functions and structs that are empty in the product build (stamp_clock, stamp_add, dst_*, LevelStamps, NetStamps,
// net_stamps_*) serve where the compiler demonstrably emits the very same code with them: straight-line kernel bodies and the
// network bodies.  Inside the search loops (phase_select, async_game, dc_phase_select, the persistent kernels' wave loops) even
// an empty local and its no-op calls changed the instruction order of the product build, so there a stamp statement is wrapped
// in IF_STAMPS(...) / IF_STAMPS_LIGHT(...) / IF_STAMPS_NET(...): the statement as written in a build with the switch, no
// tokens at all without it.  One line per stamp either way, and no preprocessor conditional in a kernel.

// ---- BB_STAMPS ---------------------------------------------------------------------------------------------------------
#ifdef BB_STAMPS
#define IF_STAMPS(...) __VA_ARGS__
constexpr bool kStamps = true;
__device__ unsigned long long g_net_stamps[NET_STAMP_WORDS];
__device__ __forceinline__ long long stamp_clock() { return clock64(); }
__device__ __forceinline__ void stamp_add(unsigned long long *stamps, int i, long long v) {
    if (stamps) atomicAdd(&stamps[i], (unsigned long long)v);
}
template <class... R>
__device__ __forceinline__ void stamp_add_all(unsigned long long *stamps, int i, long long v, R... more) { // (word, value) pairs
    stamp_add(stamps, i, v);
    if constexpr (sizeof...(more) > 0) stamp_add_all(stamps, more...);
}
__device__ __forceinline__ void stamp_wait_loads() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// Consecutive sections of one function: starts once the loads in flight have arrived; lap() waits for everything the section
// issued and returns its ticks.
struct StampSections {
    long long q0;
    __device__ __forceinline__ StampSections() {
        stamp_wait_loads();
        q0 = clock64();
    }
    __device__ __forceinline__ long long lap() {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        long long q = clock64(), dt = q - q0;
        q0 = q;
        return dt;
    }
};
__device__ __forceinline__ unsigned long long *dst_words(float *lds) { return (unsigned long long *)(lds + DC_STAMP_OFF); }
__device__ __forceinline__ void dst_zero(float *lds, int lane) {
    if (lane < STAMP_WORDS) dst_words(lds)[lane] = 0;
    __threadfence_block();
}
__device__ __forceinline__ void dst_add(float *lds, int lane, int i, long long v) {
    if (lane == 0) dst_words(lds)[i] += (unsigned long long)v;
}
__device__ __forceinline__ void dst_flush(unsigned long long *stamps, float *lds, int g) { // (one lane)
    if (stamps)
        for (int i = 0; i < STAMP_WORDS; i++) atomicAdd(&stamps[(size_t)(g & (STAMP_COPIES - 1)) * STAMP_WORDS + i], dst_words(lds)[i]);
}
#else
#define IF_STAMPS(...)
constexpr bool kStamps = false;
__device__ __forceinline__ long long stamp_clock() { return 0; }
__device__ __forceinline__ void stamp_add(unsigned long long *, int, long long) {}
__device__ __forceinline__ void dst_zero(float *, int) {}
__device__ __forceinline__ void dst_add(float *, int, int, long long) {}
__device__ __forceinline__ void dst_flush(unsigned long long *, float *, int) {}
#endif

// ---- BB_STAMPS_LIGHT ---------------------------------------------------------------------------------------------------
// What async_game measures of one call: its trailing parameter, present (and empty) in every build.
#ifdef BB_STAMPS_LIGHT
#define IF_STAMPS_LIGHT(...) __VA_ARGS__
struct LevelStamps {
    int loop = 0, levels = 0, row_load = 0, puct = 0; // ticks in the descent loops, levels descended, of those ticks: row-load wait, PUCT + argmax
};
// After the wave's async_game calls (`leader`: lane 0 of a game that was called): the game with the most levels ran the whole
// length of the call, so its loop time per level is undiluted by divergence -- that game's figures are the ones recorded.
__device__ __forceinline__ void level_stamps_flush(unsigned long long *stamps, const LevelStamps &ls, bool leader, int l64) {
    int m = ls.levels;
    for (int o = 32; o; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
    unsigned long long who = __ballot(leader && ls.levels == m);
    if (who && l64 == (int)__builtin_ctzll(who) && stamps) {
        atomicAdd(&stamps[LS_LOOP], (unsigned long long)ls.loop);
        atomicAdd(&stamps[LS_LEVELS], (unsigned long long)ls.levels);
        atomicAdd(&stamps[LS_ROW_LOAD], (unsigned long long)ls.row_load);
        atomicAdd(&stamps[LS_PUCT], (unsigned long long)ls.puct);
    }
}
#else
#define IF_STAMPS_LIGHT(...)
struct LevelStamps {};
__device__ __forceinline__ void level_stamps_flush(unsigned long long *, const LevelStamps &, bool, int) {}
#endif

// ---- BB_STAMPS_NET, BB_STAMPS_NET_SUB ------------------------------------------------------------------------------------
// net_body / net_body_x3 declare one NetStamps at entry; section(i) closes section i and starts the next.  The persistent
// kernel zeroes the workgroup's sums before its first __syncthreads and flushes them after its last.
#ifdef BB_STAMPS_NET
#define IF_STAMPS_NET(...) __VA_ARGS__
__shared__ unsigned long long s_net_stamps[NET_STAMP_WORDS];
struct NetStamps {
    long long t0 = clock64();
    __device__ __forceinline__ void stop(int i, int lane) {
        long long t = clock64();
        if (lane == 0) atomicAdd(&s_net_stamps[i], (unsigned long long)(t - t0));
    }
    __device__ __forceinline__ void section(int i, int lane) {
        stop(i, lane);
        t0 = clock64();
    }
#ifdef BB_STAMPS_NET_SUB
    __device__ __forceinline__ void sub(int i, int lane) { section(i, lane); }
#else
    __device__ __forceinline__ void sub(int, int) {}
#endif
};
__device__ __forceinline__ void net_stamps_zero() {
    if (threadIdx.x < NET_STAMP_WORDS) s_net_stamps[threadIdx.x] = 0;
}
__device__ __forceinline__ void net_stamps_flush() {
    if (threadIdx.x < NET_STAMP_WORDS) atomicAdd(&g_net_stamps[threadIdx.x], s_net_stamps[threadIdx.x]);
}
#else
#define IF_STAMPS_NET(...)
struct NetStamps {
    __device__ __forceinline__ void stop(int, int) {}
    __device__ __forceinline__ void section(int, int) {}
    __device__ __forceinline__ void sub(int, int) {}
};
__device__ __forceinline__ void net_stamps_zero() {}
__device__ __forceinline__ void net_stamps_flush() {}
#endif

// ---- BB_DIAG -----------------------------------------------------------------------------------------------------------
// (a macro: it reads the `nd` in scope, and in the default build the condition must be the literal `false`)
#ifdef BB_DIAG
#define ND_DBG(bit) (nd.dbg & (bit))
#else
#define ND_DBG(bit) false
#endif
