// net_blocks.h -- BB_NET_BLOCKS (blackbird_hip.h) for the host: the table at one shape, and what follows from a row's kind.
// Plain C++17 and nothing of HIP; tests/test_weight_blocks_cpu.py prints it from a stand-alone program.
#pragma once
#include "../../include/blackbird_hip.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

enum {
#define X(name, kind, units, per) NET_BLOCK_##name,
    BB_NET_BLOCKS(X)
#undef X
    NET_BLOCKS
};

// the table is the struct: eighteen rows, and row i's field is the i-th pointer from conv0_k on, the struct's last
static_assert(NET_BLOCKS == 18, "BB_NET_BLOCKS has a row per float block of bb_net_weights");
#define X(name, kind, units, per)                                                                                          \
    static_assert(offsetof(bb_net_weights, name) == offsetof(bb_net_weights, conv0_k) + NET_BLOCK_##name * sizeof(const float *), \
                  "BB_NET_BLOCKS is not in bb_net_weights' order at " #name);
BB_NET_BLOCKS(X)
#undef X
static_assert(sizeof(bb_net_weights) == offsetof(bb_net_weights, conv0_k) + NET_BLOCKS * sizeof(const float *), "a field without a row");

static inline const float *net_block(const bb_net_weights &w, int i) { return (&w.conv0_k)[i]; }

struct NetBlock {
    const char *name;
    int kind, units, per; // BB_BLOCK_*; `units` pieces of `per` floats
    int at;               // its first float where the blocks lie back to back
    int count() const { return units * per; }
};

struct NetBlocks {
    NetBlock b[NET_BLOCKS];
    int count; // floats of all blocks
};

static inline NetBlocks net_blocks(int C, int F, int R, int D, int A) {
    NetBlocks t = {};
#define X(name, kind, units, per) t.b[NET_BLOCK_##name] = NetBlock{#name, kind, units, per, 0};
    BB_NET_BLOCKS(X)
#undef X
    for (NetBlock &b : t.b) {
        b.at = t.count;
        t.count += b.count();
    }
    return t;
}

// per float, the trainer's variable kind: 1 trainable and in the L2 mean, 2 trainable bias, 0 moving statistics
static inline std::vector<uint8_t> net_block_kinds(const NetBlocks &t) {
    std::vector<uint8_t> kind((size_t)t.count, 1);
    for (const NetBlock &b : t.b) {
        if (b.kind == BB_BLOCK_BIAS) std::fill_n(kind.begin() + b.at, b.count(), 2);
        if (b.kind == BB_BLOCK_BN)
            for (int u = 0; u < b.units; u++) std::fill_n(kind.begin() + b.at + u * b.per + b.per / 2, b.per / 2, 0);
    }
    return kind;
}

// trainable variables whose name does not contain `bias` (the N of the L2 mean): a kernel unit is one, a batch-norm unit two
static inline int net_blocks_l2(const NetBlocks &t) {
    int n = 0;
    for (const NetBlock &b : t.b) n += b.kind == BB_BLOCK_KERNEL ? b.units : b.kind == BB_BLOCK_BN ? 2 * b.units : 0;
    return n;
}

// a block that w's shape needs and w does not give: every one but the blk_* of a network without residual blocks
static inline bool net_block_missing(const bb_net_weights &w) {
    const NetBlocks t = net_blocks(1, 1, w.R > 0, 1, 1);
    for (int i = 0; i < NET_BLOCKS; i++)
        if (t.b[i].units && !net_block(w, i)) return true;
    return false;
}
