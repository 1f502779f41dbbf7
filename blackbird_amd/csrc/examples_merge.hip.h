// examples_merge.hip.h -- the copies of a position among example records (bb_examples_fetch layout, dense games) merged into one
// training row (bb_examples_merge, bb_examples_merged_to_batch): an extension, the reference trains on every stored row.
//   key       what the network sees of the state: gs_cells(p1), gs_cells(p2), gs_player -- not gs_prev, not the header
//   groups    records with equal keys, numbered by the index of their first member in record order (rep[] ascending);
//             a record with n_children > S belongs to none: group -1 and one count in *bad, nothing it says is an address
//   sums      count (int32), zsum (int32), total (uint64), visits[A] (uint64) per group: integers only, so the order in which
//             threads arrive cannot show in a result -- there is no float atomic in this file
//   row       planes of record rep[g]; policy (float)((double)visits / (double)total), zeros when total == 0; value
//             (float)((double)zsum / (double)count).  A group of one is, bit for bit, k_examples_to_batch's row of its record.
// The table holds record indices, not keys: a thread claims an empty slot with a compare-and-swap of its own index and otherwise
// compares its key with that of the slot's owner, read from the (immutable) records -- no key is ever handed from one thread to
// another, and the owner is only ever taken from the value the atomic returned.  Everything one launch writes for another thread
// is read by a LATER launch; the launches of one call are ordered by the stream.
//   k_merge_insert   a thread per record: probe, claim or join; atomicMin of the record index per slot (the representative)
//   k_merge_count    "I am my group's first member" flags, counted per 256-record block
//   k_merge_offsets  one block: exclusive scan of the block counts in block order, n_groups (or the error word's verdict)
//   k_merge_number   the flags again, scanned inside the block in thread order: group number, rep, the first member's own sums
//   k_merge_sum      every other member added to its group: 32- and 64-bit integer atomicAdd, a thread per (record, word)
#pragma once
#include "examples.hip.h"

constexpr int32_t MERGE_EMPTY = -1;           // owner[]: hipMemsetAsync 0xFF
constexpr int32_t MERGE_NO_FIRST = 0x7F7F7F7F; // first[]: hipMemsetAsync 0x7F, above every record index (n_records <= MERGE_MAX_RECORDS)
constexpr int MERGE_MAX_RECORDS = 1 << 29;    // 2 * n_records is a table capacity that fits int32

// the table's capacity: a power of two >= 2 * n_records (load <= 1/2), at least one wave's worth
inline uint32_t merge_capacity(int n_records) {
    uint32_t cap = 64;
    while (cap < 2u * (uint32_t)n_records) cap <<= 1;
    return cap;
}
struct MergeWorkspace { // offsets in bytes into the caller's scratch memory, each a multiple of 16
    size_t owner, first, slot_of, sums, err, bytes;
    uint32_t cap;
    int blocks;
};
inline MergeWorkspace merge_workspace(int n_records) {
    auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
    MergeWorkspace w;
    w.cap = merge_capacity(n_records);
    w.blocks = (n_records + 255) / 256;
    w.owner = 0;
    w.first = w.owner + up((size_t)w.cap * 4);
    w.slot_of = w.first + up((size_t)w.cap * 4);
    w.sums = w.slot_of + up((size_t)n_records * 4);
    w.err = w.sums + up((size_t)w.blocks * 4);
    w.bytes = w.err + 16;
    return w;
}

struct MergeKey {
    uint64_t c1, c2;
    uint32_t player;
};
__device__ inline MergeKey merge_key(const uint4 &s4) {
    GridState st;
    __builtin_memcpy(&st, &s4, 16);
    return {gs_cells(st.p1), gs_cells(st.p2), (uint32_t)gs_player(st)};
}
__device__ inline uint32_t merge_hash(const MergeKey &k) { // (splitmix64's finaliser over the three words)
    uint64_t x = k.c1 * 0x9E3779B97F4A7C15ull ^ (k.c2 + 0xBF58476D1CE4E5B9ull) * 0x94D049BB133111EBull ^ ((uint64_t)k.player << 61);
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (uint32_t)x;
}

template <class G>
struct MergeRec {
    static_assert(sizeof(typename G::State) == 16, "grid state is one 16-byte load");
    static constexpr size_t OFF_VIS = sizeof(ExampleHdr) + sizeof(typename G::State), EB = OFF_VIS + 4 * G::S;
    static_assert(EB % 16 == 0 && G::A <= G::S, "records are multiples of 16 bytes and hold the visits of every action");
    __device__ static ExampleHdr hdr(const uint8_t *records, size_t r) {
        const uint4 h4 = ((const uint4 *)(records + r * EB))[0];
        ExampleHdr h;
        __builtin_memcpy(&h, &h4, 16);
        return h;
    }
    __device__ static uint4 state(const uint8_t *records, size_t r) { return ((const uint4 *)(records + r * EB))[1]; }
    __device__ static const uint32_t *visits(const uint8_t *records, size_t r) { return (const uint32_t *)(records + r * EB + OFF_VIS); }
};

// The probe loop is bounded by the capacity: a thread that finds no slot in `cap` steps (impossible at load <= 1/2 unless the
// table is damaged) sets *err, which k_merge_offsets turns into n_groups = BB_ERR_CAPACITY for the caller's next look.
template <class G>
__global__ void __launch_bounds__(256) k_merge_insert(int n_records, const uint8_t *records, uint32_t cap, int32_t *owner, int32_t *first,
                                                      int32_t *slot_of, int32_t *bad, int32_t *err) {
    using R = MergeRec<G>;
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (size_t)n_records) return;
    if (R::hdr(records, r).n_children > (uint32_t)G::S) {
        slot_of[r] = -1;
        atomicAdd(bad, 1);
        return;
    }
    const MergeKey key = merge_key(R::state(records, r));
    uint32_t slot = merge_hash(key) & (cap - 1);
    int32_t mine = -1;
    for (uint32_t i = 0; i < cap; i++, slot = (slot + 1) & (cap - 1)) {
        const int32_t was = atomicCAS(&owner[slot], MERGE_EMPTY, (int32_t)r);
        if (was != MERGE_EMPTY) { // (an owner is a well-formed record's index, put there by this launch: < n_records)
            const MergeKey other = merge_key(R::state(records, (size_t)was));
            if (other.c1 != key.c1 || other.c2 != key.c2 || other.player != key.player) continue;
        }
        atomicMin(&first[slot], (int32_t)r);
        mine = (int32_t)slot;
        break;
    }
    slot_of[r] = mine;
    if (mine < 0) atomicOr(err, 1);
}

// exclusive count of the set flags before this thread in its 256-thread block, in thread order; total: the block's count
__device__ inline int merge_block_scan(bool flag, int *s_wave, int &total) {
    const uint64_t m = __ballot(flag);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) s_wave[w] = __popcll(m);
    __syncthreads();
    int before = __popcll(m & ((1ull << lane) - 1));
    total = 0;
    for (int i = 0; i < 4; i++) {
        if (i < w) before += s_wave[i];
        total += s_wave[i];
    }
    return before;
}
__device__ inline bool merge_is_first(int n_records, size_t r, const int32_t *slot_of, const int32_t *first, int32_t &slot) {
    slot = r < (size_t)n_records ? slot_of[r] : -1;
    return slot >= 0 && first[slot] == (int32_t)r;
}

__global__ void __launch_bounds__(256) k_merge_count(int n_records, const int32_t *slot_of, const int32_t *first, int32_t *sums) {
    __shared__ int s_wave[4];
    int32_t slot;
    int total;
    merge_block_scan(merge_is_first(n_records, (size_t)blockIdx.x * 256 + threadIdx.x, slot_of, first, slot), s_wave, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums[b] -> the number of first members in blocks 0 .. b-1: 256 block counts at a time, in order, the carry in a register
__global__ void __launch_bounds__(256) k_merge_offsets(int blocks, int32_t *sums, const int32_t *err, int32_t *n_groups) {
    __shared__ int s_wave[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < blocks; base += 256) {
        const int i = base + threadIdx.x;
        const int v = i < blocks ? sums[i] : 0;
        int inc = v;
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_up(inc, d);
            if (lane >= d) inc += u;
        }
        if (lane == 63) s_wave[w] = inc;
        __syncthreads();
        int off = carry, total = 0;
        for (int j = 0; j < 4; j++) {
            if (j < w) off += s_wave[j];
            total += s_wave[j];
        }
        if (i < blocks) sums[i] = off + inc - v;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *n_groups = *err ? (int32_t)BB_ERR_CAPACITY : carry;
}

// A first member names its group and starts the group's sums with its own values (stores: the arrays need no zeroing); it
// leaves the group's number in owner[slot], which nothing reads as an owner any more.
template <class G>
__global__ void __launch_bounds__(256) k_merge_number(int n_records, const uint8_t *records, const int32_t *slot_of, const int32_t *first,
                                                      const int32_t *sums, int32_t *owner, int32_t *rep, int32_t *count, int32_t *zsum,
                                                      uint64_t *total, uint64_t *visits) {
    using R = MergeRec<G>;
    __shared__ int s_wave[4];
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    int32_t slot;
    int in_block;
    const bool is_first = merge_is_first(n_records, r, slot_of, first, slot);
    const int before = merge_block_scan(is_first, s_wave, in_block);
    if (!is_first) return;
    const size_t g = (size_t)sums[blockIdx.x] + before; // < n_records: there are no more first members than records
    const ExampleHdr h = R::hdr(records, r);
    owner[slot] = (int32_t)g;
    rep[g] = (int32_t)r;
    count[g] = 1;
    zsum[g] = h.z;
    total[g] = h.total;
    const uint32_t *vis = R::visits(records, r);
    for (int a = 0; a < G::A; a++) visits[g * G::A + a] = vis[a];
}

// A + 1 threads per record: one per action's visits, the last for group[r], count, zsum and total.
template <class G>
__global__ void __launch_bounds__(256) k_merge_sum(int n_records, const uint8_t *records, const int32_t *slot_of, const int32_t *first,
                                                   const int32_t *owner, int32_t *group, int32_t *count, int32_t *zsum, uint64_t *total,
                                                   uint64_t *visits) {
    using R = MergeRec<G>;
    constexpr int E = G::A + 1;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)n_records * E) return;
    const size_t r = t / E;
    const int e = (int)(t % E);
    const int32_t slot = slot_of[r];
    const int32_t g = slot >= 0 ? owner[slot] : -1;
    if (e == G::A) group[r] = g;
    if (slot < 0 || first[slot] == (int32_t)r) return; // no group, or the member whose values k_merge_number stored
    if (e < G::A) {
        const uint32_t v = R::visits(records, r)[e];
        if (v) atomicAdd((unsigned long long *)&visits[(size_t)g * G::A + e], (unsigned long long)v);
    } else {
        const ExampleHdr h = R::hdr(records, r);
        atomicAdd(&count[g], 1);
        if (h.z) atomicAdd(&zsum[g], (int32_t)h.z);
        if (h.total) atomicAdd((unsigned long long *)&total[g], (unsigned long long)h.total);
    }
}

// k_examples_to_batch for merged rows: row k is group index[k] (nullptr: group k) under symmetry sym[k] (nullptr: the identity).
// One thread per output element, contiguous stores, the same rules: a row whose group is outside [0, n_groups), whose sym is
// not a symmetry of the game, whose rep is outside [0, n_records) or names a record with n_children > S, or whose count is not
// positive is zeros and one count in *bad; no value becomes an index before it has been checked.
template <class G>
__global__ void __launch_bounds__(256) k_merged_to_batch(int n_records, const uint8_t *records, int n_groups, const int32_t *rep,
                                                         const int32_t *count, const int32_t *zsum, const uint64_t *total,
                                                         const uint64_t *visits, int n, const int64_t *index, const uint8_t *sym,
                                                         float *boards, float *policy, float *value, int32_t *bad) {
    using Sym = Symmetries<G::GID>;
    using R = MergeRec<G>;
    static_assert(Sym::H == G::H && Sym::W == G::W && Sym::A == G::A, "symmetry.h describes this game");
    constexpr int PL = G::H * G::W * G::C, E = PL + G::A + 1;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)n * E) return;
    const size_t k = t / E;
    const int e = (int)(t % E);
    const int64_t gi = index ? index[k] : (int64_t)k;
    const uint32_t sk = sym ? sym[k] : 0u;
    bool ok = gi >= 0 && gi < (int64_t)n_groups && sk < (uint32_t)Sym::NSYM;
    const int s = ok ? (int)sk : 0; // (only a symmetry of the game reaches the maps)
    const size_t g = ok ? (size_t)gi : 0;
    int32_t r = 0, cnt = 0;
    if (ok) {
        r = rep[g];
        cnt = count[g];
        ok = r >= 0 && r < n_records && cnt > 0;
    }
    typename G::State st = {};
    if (ok) {
        const uint4 s4 = R::state(records, (size_t)r);
        __builtin_memcpy(&st, &s4, 16);
        ok = R::hdr(records, (size_t)r).n_children <= (uint32_t)G::S;
    }
    if (e < PL) {
        if (!boards) return;
        const int cell = Sym::cell_inv(s, e / G::C); // the cell whose planes land on cell e / C
        int8_t v[G::C] = {};
        if (ok) G::encode_cell(st, cell / G::W, cell % G::W, v);
        boards[k * PL + e] = (float)v[e % G::C];
    } else if (e < PL + G::A) {
        if (!policy) return;
        const int a = e - PL, from = Sym::action_inv(s, a); // (< A)
        float p = 0.f;
        if (ok) {
            const uint64_t tot = total[g];
            if (tot) p = (float)((double)visits[g * G::A + from] / (double)tot);
        }
        policy[k * G::A + a] = p;
    } else { // the row's last element: the mean outcome, and the row's word in the count of rejected rows
        if (value) value[k] = ok ? (float)((double)zsum[g] / (double)cnt) : 0.f;
        if (!ok && bad) atomicAdd(bad, 1);
    }
}
