// starts.h -- host side of bb_selfplay_set_starts (include/blackbird_hip.h): the argument checks, the reading of the device's
// verdicts and the bookkeeping of the table an engine owns.  No HIP here: what touches the device comes in through StartsOps, so a
// stand-alone program can drive the same code over the C heap under a sanitizer (tests/test_selfplay_starts_cpu.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

// one verdict per state, written by k_check_starts (tree.hip.h, tree_dc.hip.h); the order is the order the reasons are looked at
enum { BB_START_OK = 0, BB_START_FINISHED = 1, BB_START_NO_MOVE = 2, BB_START_TOO_WIDE = 3 };
// what starts_replace answers; the entry point maps them to bb_status
enum { STARTS_DONE = 0, STARTS_BAD_ARG = 1, STARTS_NO_FIT = 2, STARTS_DEVICE = 3, STARTS_REFUSED = 4 };

static inline const char *starts_reason_text(int verdict) {
    switch (verdict) {
    case BB_START_FINISHED: return "the game is already over there (Winner() is not None)";
    case BB_START_NO_MOVE: return "it has no legal move";
    case BB_START_TOO_WIDE: return "it has more legal moves than a tree node holds (bb_game_info.S)";
    default: return "unknown verdict";
    }
}

// Before any device call.  n and states first, the engine last: what is wrong with the table is said even without an engine.
static inline int starts_check_args(bool have_engine, int n, const void *states, char *msg, size_t cap) {
    if (n < 0) {
        snprintf(msg, cap, "bb_selfplay_set_starts: n = %d is negative", n);
        return STARTS_BAD_ARG;
    }
    if (n > 0 && !states) {
        snprintf(msg, cap, "bb_selfplay_set_starts: states is NULL with n = %d", n);
        return STARTS_BAD_ARG;
    }
    if (!have_engine) {
        snprintf(msg, cap, "bb_selfplay_set_starts: null engine");
        return STARTS_BAD_ARG;
    }
    return STARTS_DONE;
}

// The first refused state of a verdict array: its index (-1: none) and its verdict.
static inline int starts_first_refused(const uint8_t *verdict, int n, int *reason) {
    for (int i = 0; i < n; i++)
        if (verdict[i] != BB_START_OK) {
            *reason = verdict[i];
            return i;
        }
    *reason = BB_START_OK;
    return -1;
}

struct StartsTable {
    void *dev = nullptr; // n packed states in device memory, owned
    int n = 0;
};

struct StartsOps { // the device side.  Every function: 0, or nonzero on failure (alloc: 1 = does not fit, else another failure)
    void *ctx;
    int (*alloc)(void *ctx, size_t bytes, void **out);
    int (*upload)(void *ctx, void *dst, const void *src, size_t bytes);
    int (*check)(void *ctx, const void *dev_states, int n, uint8_t *verdict_out); // k_check_starts; verdict_out[n] is host memory
    void (*release)(void *ctx, void *p);
};

// Replace the table by a checked copy of states[n] (n == 0: by none).  The new copy is made and checked first: whatever goes
// wrong, `t` is what it was.
static inline int starts_replace(StartsTable &t, int n, const void *states, size_t state_bytes, const StartsOps &ops, char *msg, size_t cap) {
    if (n == 0) {
        if (t.dev) ops.release(ops.ctx, t.dev);
        t = StartsTable();
        return STARTS_DONE;
    }
    const size_t bytes = (size_t)n * state_bytes;
    void *fresh = nullptr;
    if (int rc = ops.alloc(ops.ctx, bytes, &fresh)) {
        snprintf(msg, cap, "bb_selfplay_set_starts: a table of %d states (%zu bytes) %s", n, bytes,
                 rc == 1 ? "does not fit the device's free memory" : "could not be allocated");
        return rc == 1 ? STARTS_NO_FIT : STARTS_DEVICE;
    }
    std::vector<uint8_t> verdict((size_t)n, (uint8_t)BB_START_OK);
    if (ops.upload(ops.ctx, fresh, states, bytes) || ops.check(ops.ctx, fresh, n, verdict.data())) {
        ops.release(ops.ctx, fresh);
        snprintf(msg, cap, "bb_selfplay_set_starts: copying or checking the table failed on the device");
        return STARTS_DEVICE;
    }
    int reason = BB_START_OK;
    const int bad = starts_first_refused(verdict.data(), n, &reason);
    if (bad >= 0) {
        ops.release(ops.ctx, fresh);
        snprintf(msg, cap, "bb_selfplay_set_starts: state %d refused: %s (reason %d); the previous table stays", bad,
                 starts_reason_text(reason), reason);
        return STARTS_REFUSED;
    }
    if (t.dev) ops.release(ops.ctx, t.dev);
    t.dev = fresh;
    t.n = n;
    return STARTS_DONE;
}
