// host_common.hip.h -- what every host file of engine.hip uses: the thread's last error (fail, HIPCHK), the HIP side of dev_mem.h,
// the staging buffer of an entry point, grid sizing and the switch over the games.
#pragma once
#include "dev_mem.h"

#include <cassert>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

static thread_local std::string g_err;
static int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIPCHK(x)                                                                                      \
    do {                                                                                               \
        hipError_t _e = (x);                                                                           \
        if (_e != hipSuccess) return fail(BB_ERR_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(_e), \
                                          __FILE__, __LINE__);                                         \
    } while (0)

extern "C" const char *bb_last_error(void) { return g_err.c_str(); }

extern "C" int bb_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---- the HIP side of dev_mem.h: the only hipMalloc / hipFree / stream and event creation of the library (and starts_ops) ------
static const DevOps HIP_OPS = {
    nullptr,
    [](void *, size_t bytes, void **out) -> int { return (int)hipMalloc(out, bytes); },
    [](void *, void *p) { (void)hipFree(p); },
    [](void *, void *p, size_t bytes, void *stream) -> int { return (int)hipMemsetAsync(p, 0, bytes, (hipStream_t)stream); },
    [](void *, void *dst, const void *src, size_t bytes) -> int { return (int)hipMemcpy(dst, src, bytes, hipMemcpyDefault); },
    [](void *, void **out) -> int { return (int)hipStreamCreateWithFlags((hipStream_t *)out, hipStreamNonBlocking); },
    [](void *, void *stream) { (void)hipStreamDestroy((hipStream_t)stream); },
    [](void *, bool timing, void **out) -> int {
        return (int)(timing ? hipEventCreate((hipEvent_t *)out) : hipEventCreateWithFlags((hipEvent_t *)out, hipEventDisableTiming));
    },
    [](void *, void *event) { (void)hipEventDestroy((hipEvent_t)event); },
    [](void *, int rc) -> const char * { return hipGetErrorString((hipError_t)rc); },
    [](void *, const char *msg) -> int { return fail(BB_ERR_HIP, "%s", msg); },
};
// device scratch of one call, released on scope exit
template <class T>
struct Staged : StagedOn<T> {
    Staged() : StagedOn<T>(HIP_OPS) {}
};
// what a create function builds its object in: every return before release() destroys it, as the caller's destroy would
template <class T, int (*Destroy)(T *)>
struct Destroyer {
    void operator()(T *p) const { (void)Destroy(p); }
};
template <class T, int (*Destroy)(T *)>
using Building = std::unique_ptr<T, Destroyer<T, Destroy>>;

// what both scorers (bb_trainer_eval*, bb_examples_score) ask of their outputs in the same words: a place for the bb_eval_totals
static int score_outputs_ok(const void *totals) {
    return !totals || (uintptr_t)totals % 8 ? fail(BB_ERR_ARG, "totals_out must be an 8-byte aligned device pointer") : BB_OK;
}

static inline int nblk(size_t n, int per = 256) { return (int)((n + per - 1) / per); }
// grid and block of every one-wave-per-slot kernel (search_wave*.hip.h, selfplay_wave.hip.h): <<<SW_GRID(d), 0, stream>>>
#define SW_GRID(d) nblk((d).n_slots, SW_WAVES), 64 * SW_WAVES

#define GAME_SWITCH(game, ...)                                                   \
    switch (game) {                                                              \
    case BB_GAME_CONNECT4: { using G = Connect4; __VA_ARGS__; }                  \
    case BB_GAME_TICTACTOE: { using G = TicTacToe; __VA_ARGS__; }                \
    case BB_GAME_DRAGONCHESS: { using G = DragonChess; __VA_ARGS__; }            \
    default: return fail(BB_ERR_ARG, "unknown game %d", game);                   \
    }
