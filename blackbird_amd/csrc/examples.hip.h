// examples.hip.h -- example records (bb_examples_fetch layout: ExampleHdr, packed state, u32 visits[S], compact games:
// u16 action[S]) -> the three float32 tensors the training loss takes (bb_examples_to_batch):
//     boards [n][H][W][C]  AsInputArray planes of the record's state (the game's encode_cell)
//     policy [n][A]        (float)((double)visits / (double)total): divided in double and rounded once, as the host path
//                          does (float64 visits / total, then float32); zeros when total == 0 (the terminal example)
//     value  [n]           z
// Row k comes from record index[k] (index == nullptr: record k).  A row whose index is outside [0, n_records), whose
// n_children exceeds S or (compact games) one of whose actions is >= A is written as zeros and counted in *bad: nothing of
// what a record says is used as an address before it has been checked.
// sym (bb_examples_to_batch_sym; nullptr: the identity everywhere): row k is the row of the position transformed by the game's
// symmetry sym[k] (symmetry.h) -- the same values, a cell's planes at the cell's image and an action's share at the action's image.
// A row whose sym[k] is not a symmetry of the game is a malformed row like the others: zeros and one count, and no map sees it.
#pragma once
#include "symmetry.h"
#include "tree.hip.h"

// records are read in 16-byte units (headers and states whole); they are multiples of 16 bytes (bb_examples_fetch_games)
static_assert(sizeof(ExampleHdr) == 16, "example header is one 16-byte load");

// One row of a batch from the dense games' records, checked: record index[k] (nullptr: record k) under symmetry sym[k] (nullptr:
// the identity).  The header and the state are one 16-byte load each, made only once the index and the symmetry have passed;
// a caller that uses one of them only leaves the other load dead.  !ok: a malformed row -- s is 0, nothing was read, and
// example_plane, example_share and example_value answer 0.  What k_examples_to_batch writes and what the training kernels
// read straight from the records (train.hip.h) are these functions, so the two cannot drift apart.
template <class G>
struct ExampleRow {
    static constexpr int PL = G::H * G::W * G::C;
    static constexpr size_t OFF_VIS = sizeof(ExampleHdr) + sizeof(typename G::State), EB = OFF_VIS + 4 * G::S;
    static_assert(sizeof(typename G::State) == 16, "grid state is one 16-byte load");
    static_assert(EB % 16 == 0, "records are multiples of 16 bytes");
    static_assert(G::A <= G::S, "a dense record holds the visits of every action");
    bool ok;
    int s; // (only a symmetry of the game reaches the maps)
    ExampleHdr h;
    typename G::State st;
    const uint8_t *rec;
};

template <class G>
__device__ __forceinline__ ExampleRow<G> example_row(int n_records, const uint8_t *records, const int64_t *index, const uint8_t *sym,
                                                     size_t k) {
    using Sym = Symmetries<G::GID>;
    static_assert(Sym::H == G::H && Sym::W == G::W && Sym::A == G::A, "symmetry.h describes this game");
    const int64_t r = index ? index[k] : (int64_t)k;
    const uint32_t sk = sym ? sym[k] : 0u;
    ExampleRow<G> row = {};
    row.ok = r >= 0 && r < (int64_t)n_records && sk < (uint32_t)Sym::NSYM;
    row.s = row.ok ? (int)sk : 0;
    row.rec = records + (size_t)(row.ok ? r : 0) * ExampleRow<G>::EB;
    if (row.ok) {
        const uint4 h4 = ((const uint4 *)row.rec)[0], s4 = ((const uint4 *)row.rec)[1];
        __builtin_memcpy(&row.h, &h4, 16);
        __builtin_memcpy(&row.st, &s4, 16);
        row.ok = row.h.n_children <= (uint32_t)G::S;
    }
    return row;
}

// element e of the row's planes [H][W][C]: a thread finds the cell its element comes FROM through the symmetry's inverse map
template <class G>
__device__ __forceinline__ float example_plane(const ExampleRow<G> &row, int e) {
    const int cell = Symmetries<G::GID>::cell_inv(row.s, e / G::C); // the cell whose planes land on cell e / C
    int8_t v[G::C] = {};
    if (row.ok) G::encode_cell(row.st, cell / G::W, cell % G::W, v);
    return (float)v[e % G::C];
}

// entry a of the row's policy label: divided in double and rounded once; zeros when total == 0 (the terminal example)
template <class G>
__device__ __forceinline__ float example_share(const ExampleRow<G> &row, int a) {
    const int from = Symmetries<G::GID>::action_inv(row.s, a); // (both < A <= S: inside the record's visits)
    float p = 0.f;
    if (row.ok && row.h.total) p = (float)((double)((const uint32_t *)(row.rec + ExampleRow<G>::OFF_VIS))[from] / (double)row.h.total);
    return p;
}

template <class G>
__device__ __forceinline__ float example_value(const ExampleRow<G> &row) {
    return row.ok ? (float)row.h.z : 0.f;
}

// Dense games (slot i == action i): one thread per output element, rows back to back -- a 256-thread block covers a few
// records (Connect4: 134 floats per row, TicTacToe: 37), a wave's stores are contiguous within each of the three outputs.
// The lanes of a row read the same addresses (one fetch, broadcast); the stores stay as they are under a symmetry.
// One kernel with and without sym: the only branch is the uniform one around the load of sym[k], the maps run with 0 otherwise.
template <class G>
__global__ void __launch_bounds__(256) k_examples_to_batch(int n_records, const uint8_t *records, int n, const int64_t *index,
                                                           const uint8_t *sym, float *boards, float *policy, float *value,
                                                           int32_t *bad) {
    constexpr int PL = ExampleRow<G>::PL, E = PL + G::A + 1;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)n * E) return;
    const size_t k = t / E;
    const int e = (int)(t % E);
    const ExampleRow<G> row = example_row<G>(n_records, records, index, sym, k);
    if (e < PL) {
        if (!boards) return;
        boards[k * PL + e] = example_plane<G>(row, e);
    } else if (e < PL + G::A) {
        if (!policy) return;
        policy[k * G::A + (e - PL)] = example_share<G>(row, e - PL);
    } else { // the row's last element: z, and the row's word in the count of rejected rows
        if (value) value[k] = example_value<G>(row);
        if (!row.ok && bad) atomicAdd(bad, 1);
    }
}

// DragonChess (compact child lists: visits[j] belongs to action[j], j < n_children): one block per record.  The record
// (960 bytes) comes in as 60 16-byte loads; the 4032-wide policy row is built in LDS -- zeroed, then up to S entries
// scattered -- and streamed out with 16-byte stores, so global memory sees every float once and in order.  The planes
// (64 cells x 17) take the same way through LDS: a cell's 17 values are written by its own lane, rows of 17 floats, an odd
// stride, so that the 64 lanes fall on different banks.  DragonChess has no symmetry but the identity: a row with any other
// sym[k] is treated as a row whose index is out of range.
__global__ void __launch_bounds__(256) k_dc_examples_to_batch(int n_records, const uint8_t *records, const int64_t *index,
                                                              const uint8_t *sym, float *boards, float *policy, float *value,
                                                              int32_t *bad) {
    using G = DragonChess;
    constexpr int S = G::S, A = G::A, PL = G::H * G::W * G::C;
    constexpr int EB = (int)(sizeof(ExampleHdr) + sizeof(DCState)) + 4 * S + 2 * S;
    constexpr int OFF_VIS = (int)(sizeof(ExampleHdr) + sizeof(DCState)), OFF_ACT = OFF_VIS + 4 * S;
    static_assert(EB % 16 == 0 && A % 4 == 0 && PL % 4 == 0, "16-byte loads and stores");
    __shared__ uint4 s_rec[EB / 16];
    __shared__ float4 s_pol[A / 4];
    __shared__ float4 s_brd[PL / 4];
    const int tid = threadIdx.x;
    const size_t k = blockIdx.x;
    const int64_t r = index ? index[k] : (int64_t)k;
    const bool in_range = r >= 0 && r < (int64_t)n_records && (sym ? sym[k] : 0) < Symmetries<G::GID>::NSYM; // (the same for the whole block)
    if (in_range && tid < EB / 16) s_rec[tid] = ((const uint4 *)(records + (size_t)r * EB))[tid];
    for (int i = tid; i < A / 4; i += 256) s_pol[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = tid; i < PL / 4; i += 256) s_brd[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    const uint8_t *rec = (const uint8_t *)s_rec;
    const ExampleHdr *h = (const ExampleHdr *)rec;
    const uint32_t nch = in_range ? h->n_children : (uint32_t)S + 1u;
    const uint32_t total = in_range ? h->total : 0u;
    const bool mine = in_range && (uint32_t)tid < nch && tid < S; // this lane's child entry
    const uint32_t act = mine ? ((const uint16_t *)(rec + OFF_ACT))[tid] : 0u;
    const bool ok = !__syncthreads_or((nch > (uint32_t)S) | (act >= (uint32_t)A));
    if (ok) {
        if (mine && total) ((float *)s_pol)[act] = (float)((double)((const uint32_t *)(rec + OFF_VIS))[tid] / (double)total);
        if (tid < G::H * G::W) {
            int8_t v[G::C];
            G::encode_cell(*(const DCState *)(rec + sizeof(ExampleHdr)), tid >> 3, tid & 7, v);
            for (int c = 0; c < G::C; c++) ((float *)s_brd)[tid * G::C + c] = (float)v[c];
        }
    }
    __syncthreads();
    if (policy)
        for (int i = tid; i < A / 4; i += 256) ((float4 *)(policy + k * A))[i] = s_pol[i];
    if (boards)
        for (int i = tid; i < PL / 4; i += 256) ((float4 *)(boards + k * PL))[i] = s_brd[i];
    if (tid == 0) {
        if (value) value[k] = ok ? (float)h->z : 0.f;
        if (!ok && bad) atomicAdd(bad, 1);
    }
}
