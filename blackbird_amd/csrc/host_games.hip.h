// host_games.hip.h -- the entry points that need no engine: a game's figures and the stateless batched game ops.
#pragma once
template <class G>
static void fill_info(bb_game_info *o) {
    o->H = G::H;
    o->W = G::W;
    o->C = G::C;
    o->A = G::A;
    o->S = G::S;
    o->state_bytes = (int)sizeof(typename G::State);
    o->dense = 1;
    o->example_bytes = (int)(sizeof(ExampleHdr) + sizeof(typename G::State) + 4 * G::S);
}

extern "C" int bb_game_info_get(int game, bb_game_info *out) {
    if (!out) return fail(BB_ERR_ARG, "null out");
    switch (game) {
    case BB_GAME_CONNECT4: fill_info<Connect4>(out); return BB_OK;
    case BB_GAME_TICTACTOE: fill_info<TicTacToe>(out); return BB_OK;
    case BB_GAME_DRAGONCHESS:
        fill_info<DragonChess>(out);
        out->dense = 0;
        out->example_bytes = (int)(sizeof(ExampleHdr) + sizeof(DCState) + 4 * DragonChess::S + 2 * DragonChess::S);
        return BB_OK;
    default: return fail(BB_ERR_ARG, "unknown or unsupported game %d", game);
    }
}

extern "C" int bb_game_symmetries(int game) {
    const int n = game_symmetries(game); // (symmetry.h)
    return n > 0 ? n : fail(BB_ERR_ARG, "unknown or unsupported game %d", game);
}

// ---- stateless batched game ops ------------------------------------------------------------------
template <class G>
static int game_legal(int n, const void *states, uint8_t *out) {
    Staged<typename G::State> ds;
    Staged<uint8_t> dout;
    if (ds.alloc((size_t)n) || dout.alloc((size_t)n * G::A)) return BB_ERR_HIP;
    if (int rc = ds.from_host(states)) return rc;
    Launch<G>::legal(n, ds.get(), dout.get());
    HIPCHK(hipGetLastError());
    return dout.to_host(out);
}
template <class G>
static int game_apply(int n, void *states, const int32_t *actions, int32_t *status) {
    Staged<typename G::State> ds;
    Staged<int32_t> da, dst;
    if (ds.alloc((size_t)n) || da.alloc((size_t)n) || dst.alloc((size_t)n)) return BB_ERR_HIP;
    if (int rc = ds.from_host(states)) return rc;
    if (int rc = da.from_host(actions)) return rc;
    k_game_apply<G><<<nblk(n), 256>>>(n, ds.get(), da.get(), dst.get());
    HIPCHK(hipGetLastError());
    if (int rc = ds.to_host(states)) return rc;
    return status ? dst.to_host(status) : BB_OK;
}
template <class G>
static int game_winner(int n, const void *states, const int32_t *prev, int8_t *out) {
    Staged<typename G::State> ds;
    Staged<int32_t> dp;
    Staged<int8_t> dout;
    if (ds.alloc((size_t)n) || dp.alloc((size_t)n) || dout.alloc((size_t)n)) return BB_ERR_HIP;
    if (int rc = ds.from_host(states)) return rc;
    if (prev)
        if (int rc = dp.from_host(prev)) return rc;
    k_game_winner<G><<<nblk(n), 256>>>(n, ds.get(), prev ? dp.get() : nullptr, dout.get());
    HIPCHK(hipGetLastError());
    return dout.to_host(out);
}
template <class G>
static int game_encode(int n, const void *states, int8_t *out) {
    Staged<typename G::State> ds;
    Staged<int8_t> dout;
    if (ds.alloc((size_t)n) || dout.alloc((size_t)n * G::H * G::W * G::C)) return BB_ERR_HIP;
    if (int rc = ds.from_host(states)) return rc;
    Launch<G>::encode(n, ds.get(), dout.get());
    HIPCHK(hipGetLastError());
    return dout.to_host(out);
}

extern "C" int bb_game_legal(int game, int n, const void *states, uint8_t *legal_out) {
    if (n == 0) return BB_OK; // an empty batch is a no-op
    if (n < 0 || !states || !legal_out) return fail(BB_ERR_ARG, "bad arguments");
    GAME_SWITCH(game, return game_legal<G>(n, states, legal_out));
}
extern "C" int bb_game_apply(int game, int n, void *states, const int32_t *actions, int32_t *status_out) {
    if (n == 0) return BB_OK;
    if (n < 0 || !states || !actions) return fail(BB_ERR_ARG, "bad arguments");
    GAME_SWITCH(game, return game_apply<G>(n, states, actions, status_out));
}
extern "C" int bb_game_winner(int game, int n, const void *states, const int32_t *prev, int8_t *winner_out) {
    if (n == 0) return BB_OK;
    if (n < 0 || !states || !winner_out) return fail(BB_ERR_ARG, "bad arguments");
    GAME_SWITCH(game, return game_winner<G>(n, states, prev, winner_out));
}
extern "C" int bb_game_encode(int game, int n, const void *states, int8_t *planes_out) {
    if (n == 0) return BB_OK;
    if (n < 0 || !states || !planes_out) return fail(BB_ERR_ARG, "bad arguments");
    GAME_SWITCH(game, return game_encode<G>(n, states, planes_out));
}
extern "C" int bb_game_initial(int game, void *state_out) {
    if (!state_out) return fail(BB_ERR_ARG, "null out");
    GAME_SWITCH(game, {
        typename G::State s = G::initial();
        memcpy(state_out, &s, sizeof s);
        return BB_OK;
    });
}
