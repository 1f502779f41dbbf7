// examples_score.hip.h -- score example records with the network an ENGINE holds (bb_examples_score): whatever launch_net runs
// for it -- the fused 16-filter tower or the launch-per-layer network, split-operand or float32-MFMA form, any game.  Two kernels
// around the engine's own network launch, per chunk of rows:
//   k_score_gather  one thread per row: the record is checked, its packed state copied into a contiguous G::State array
//   (launch_net)    value[chunk], logits[chunk][A] of those states: no noise, no keys, no evaluation cache
//   k_score_rows    one wave per row, four rows per workgroup: value, squared error, cross entropy against the record's own label
//                   and the flags byte
// and k_train_eval_totals (train_eval.hip.h) once over the finished rows.
//
// Records: the bb_examples_fetch layout (examples.hip.h) -- ExampleHdr, packed state, u32 visits[S], compact games u16 action[S].
// Row k of a call is record index[k] (nullptr: record k).  A row is malformed, as example_row / k_dc_examples_to_batch define it,
// when its index is outside [0, n_records), when n_children > S, or (DragonChess) when an action[j], j < n_children, is >= A.
// k_score_gather decides that once per row and leaves the verdict in ok[k]; a malformed row gets the game's initial state (the
// network kernels never see unchecked bytes), ok 0 and one integer atomicAdd on *bad.  k_score_rows reads a record only where
// ok[k] says that it passed: nothing a record says is used as an address before.  A malformed row is {0, 0, 0}, flags 0.
//
// Per row: a scored row as train_eval.hip.h states it (score_value_part, score_policy_serial: the figures, their orders and the
// flags), with value = the engine's, unchanged, target = z and pi = (float)((double)visits / (double)total) -- example_share's
// division --, 0 when total == 0.
//
// Sum orders (float32, no float atomics: the same input gives the same bits).
//   Dense games (A <= 16): lane 0 of the row's wave calls score_policy_serial, as k_train_eval does.
//   DragonChess (A = 4032): the same figures and flags over the whole wave.  The row is read as 1008 16-byte groups; lane l takes groups l, l + 64, ... (16 passes, the last one
//   lanes 0..47 only), the four logits of a group in action order, so the lane's actions ascend.  The lane's maximum (and its
//   first position: strict >) and the lane's sum of expf follow that order; the 64 lanes are then combined by one xor butterfly
//   (offsets 32, 16, 8, 4, 2, 1; float addition commutes, so every lane ends with the same bits; of two equal maxima the smaller
//   action wins, so the result is the row's first maximum).  The row's logits stay in registers between the two passes.
//   The <= 144 children take three 64-lane passes (j = lane, lane + 64, lane + 128, as the tree kernels walk a node's edges):
//   the lane's ce part is an fmaf chain over its children in that order, then the same butterfly.  The label's first maximum is
//   the child with the largest share, ties to the smallest action id wherever it stands in the list: the argmax of the dense row
//   bb_examples_to_batch writes, without forming that row.  Duplicate actions are no error; every entry counts.
// No LDS: a row lives in one wave's registers, all exchanges are cross-lane moves.
#pragma once
#include "examples.hip.h"
#include "train_eval.hip.h"

template <class G>
struct ScoreRecord { // where the parts of a record lie
    static constexpr bool COMPACT = G::GID == BB_GAME_DRAGONCHESS;
    static constexpr size_t SB = sizeof(typename G::State);
    static constexpr size_t OFF_VIS = sizeof(ExampleHdr) + SB, OFF_ACT = OFF_VIS + 4 * G::S;
    static constexpr size_t EB = OFF_ACT + (COMPACT ? 2 * G::S : 0);
    static_assert(SB % 16 == 0 && EB % 16 == 0, "headers, states and records are read in 16-byte units");
    static_assert(COMPACT || G::A <= G::S, "a dense record holds the visits of every action");
};

// rows first .. first + n of the call -> states[0 .. n), ok[0 .. n)
template <class G>
__global__ void __launch_bounds__(256) k_score_gather(int n_records, const uint8_t *__restrict__ records, int n, int first,
                                                      const int64_t *__restrict__ index, typename G::State *__restrict__ states,
                                                      uint8_t *__restrict__ ok_out, int32_t *bad) {
    using SR = ScoreRecord<G>;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int64_t r = index ? index[(size_t)first + k] : (int64_t)first + k;
    bool ok = r >= 0 && r < (int64_t)n_records;
    const uint8_t *rec = records + (size_t)(ok ? r : 0) * SR::EB;
    if (ok) {
        const uint4 h4 = ((const uint4 *)rec)[0];
        ExampleHdr h;
        __builtin_memcpy(&h, &h4, 16);
        ok = h.n_children <= (uint32_t)G::S;
        if constexpr (SR::COMPACT) {
            if (ok) {
                const uint16_t *act = (const uint16_t *)(rec + SR::OFF_ACT);
                for (uint32_t j = 0; j < h.n_children; j++) ok = ok && act[j] < (uint32_t)G::A;
            }
        }
    }
    uint4 *dst = (uint4 *)(states + k);
    if (ok) {
        const uint4 *src = (const uint4 *)(rec + sizeof(ExampleHdr));
        for (int i = 0; i < (int)(SR::SB / 16); i++) dst[i] = src[i];
    } else {
        const typename G::State s0 = G::initial();
        states[k] = s0;
        if (bad) atomicAdd(bad, 1);
    }
    ok_out[k] = ok ? 1 : 0;
}

__device__ __forceinline__ float score_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// of two (value, action) pairs the larger value, of equal values the smaller action; a pair with action < 0 is no candidate
__device__ __forceinline__ void score_take_first_max(float &v, int &a, float ov, int oa) {
    if (oa >= 0 && (a < 0 || ov > v || (ov == v && oa < a))) {
        v = ov;
        a = oa;
    }
}
__device__ __forceinline__ void score_wave_first_max(float &v, int &a) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(v, off);
        const int oa = __shfl_xor(a, off);
        score_take_first_max(v, a, ov, oa);
    }
}

// value[n], logits[n][A]: the engine's outputs for rows first .. first + n; rows_out / flags_out: the call's, from row 0
template <class G>
__global__ void __launch_bounds__(256) k_score_rows(int n_records, const uint8_t *__restrict__ records, int n, int first,
                                                    const int64_t *__restrict__ index, const uint8_t *__restrict__ ok_in,
                                                    const float *__restrict__ value, const float *__restrict__ logits,
                                                    float *__restrict__ rows_out, uint8_t *__restrict__ flags_out) {
    using SR = ScoreRecord<G>;
    constexpr int A = G::A;
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6); // (the same for the whole wave)
    if (k >= n) return;
    float out[3] = {0.f, 0.f, 0.f};
    int flags = 0;
    if (ok_in[k]) { // the record passed k_score_gather's checks: its index is in range, its counts and actions are bounded
        const int64_t r = index ? index[(size_t)first + k] : (int64_t)first + k;
        const uint8_t *rec = records + (size_t)r * SR::EB;
        const uint4 h4 = ((const uint4 *)rec)[0];
        ExampleHdr h;
        __builtin_memcpy(&h, &h4, 16);
        const uint32_t *vis = (const uint32_t *)(rec + SR::OFF_VIS);
        score_value_part(value[k], (float)h.z, out, flags);
        if constexpr (!SR::COMPACT) {
            static_assert(SR::COMPACT || A <= 16, "the serial form: a handful of actions");
            if (lane == 0) {
                const float *lg = logits + (size_t)k * A;
                const uint32_t total = h.total;
                score_policy_serial<A>([=](int a) { return lg[a]; },
                                       [=](int a) { return total ? (float)((double)vis[a] / (double)total) : 0.f; }, out, flags);
            }
        } else {
            static_assert(!SR::COMPACT || (A % 4 == 0 && G::S <= 192), "16-byte groups; three passes over the children");
            constexpr int NG = A / 4, PASSES = (NG + 63) / 64;
            const float4 *lg4 = (const float4 *)(logits + (size_t)k * A);
            float4 q[PASSES];
            float mx = -INFINITY;
            int amax = -1;
#pragma unroll
            for (int t = 0; t < PASSES; t++) {
                const int g = lane + 64 * t;
                if (g < NG) {
                    q[t] = lg4[g];
                    const float e[4] = {q[t].x, q[t].y, q[t].z, q[t].w};
#pragma unroll
                    for (int c = 0; c < 4; c++)
                        if (amax < 0 || e[c] > mx) { mx = e[c]; amax = 4 * g + c; }
                } else {
                    q[t] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY); // (expf gives 0: nothing is added)
                }
            }
            score_wave_first_max(mx, amax);
            float sum = 0.f;
#pragma unroll
            for (int t = 0; t < PASSES; t++)
                if (lane + 64 * t < NG) sum += ((expf(q[t].x - mx) + expf(q[t].y - mx)) + expf(q[t].z - mx)) + expf(q[t].w - mx);
            sum = score_wave_sum(sum);
            const float lse = logf(sum);
            const uint16_t *act = (const uint16_t *)(rec + SR::OFF_ACT);
            const float *lg = logits + (size_t)k * A;
            float acc = 0.f, top_pi = 0.f;
            int best_pi = -1;
            bool any = false;
#pragma unroll
            for (int p = 0; p < 3; p++) {
                const uint32_t j = (uint32_t)(lane + 64 * p);
                if (j < h.n_children) { // (n_children <= S and act[j] < A: k_score_gather)
                    const uint32_t v = vis[j];
                    const int a = act[j];
                    const float pi = h.total ? (float)((double)v / (double)h.total) : 0.f;
                    any = any || (h.total != 0 && v != 0);
                    acc = __builtin_fmaf(pi, (lg[a] - mx) - lse, acc);
                    score_take_first_max(top_pi, best_pi, pi, a);
                }
            }
            acc = score_wave_sum(acc);
            score_wave_first_max(top_pi, best_pi);
            if (__any(any)) {
                out[2] = -acc;
                flags |= BB_ROW_HAS_POLICY;
                if (best_pi == amax) flags |= BB_ROW_TOP1;
            }
        }
    }
    if (lane == 0) {
        const size_t row = (size_t)first + k;
        rows_out[row * 3] = out[0];
        rows_out[row * 3 + 1] = out[1];
        rows_out[row * 3 + 2] = out[2];
        flags_out[row] = (uint8_t)flags;
    }
}
