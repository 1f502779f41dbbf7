/*
 * include/blackbird_hip.h -- C ABI of libblackbird_hip.so (MI355X / gfx950).
 *
 * The reference (ZackAttack614/BlackBird) is pure Python and has no FFI of its own; its drop-in
 * boundary for the self-play hot path is the Python API
 *     Blackbird.GenerateTrainingSamples   (src/Blackbird.py:219-268)
 *     MCTS.FindMove / MoveRoot / DropRoot (src/MCTS.py:146-225)
 *     Network.getEvaluation / getPolicy   (src/Network.py:48-64)
 *     GameState.LegalActions / ApplyAction / Winner / AsInputArray
 *                                         (src/GameState.py:1-28, Connect4.py, TicTacToe.py, DragonChess.py)
 * The modules under blackbird_amd/ mirror those classes and binds the entry points below with ctypes
 * (INTEGRATION.md shows the binding).  Each entry point cites the reference code it replaces.
 *
 * Conventions: every function returns 0 on success or a negative bb_status; bb_last_error()
 * gives the message.  All buffers are caller-allocated; a pointer may be host or device memory
 * (copies use hipMemcpyDefault).  An engine is bound to one GPU and is not thread-safe (the
 * reference is single-threaded).  There is no CPU fallback: without a GPU every compute entry
 * point fails with BB_ERR_HIP.
 */
#ifndef BLACKBIRD_HIP_H
#define BLACKBIRD_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    BB_OK = 0,
    BB_ERR_ARG = -1,      /* ValueError in the reference (bad nGames, no stop rule, ...) */
    BB_ERR_HIP = -2,      /* HIP runtime failure / no device */
    BB_ERR_STATE = -3,    /* AssertionError: tree root does not match the state (MCTS.py:193) */
    BB_ERR_NAN = -4,      /* ValueError: probabilities contain NaN (MCTS.py:336-338, 1 sim on a fresh root) */
    BB_ERR_CAPACITY = -5, /* node pool / example store exhausted */
    BB_ERR_WEIGHTS = -6   /* network evaluator requested before bb_load_weights */
} bb_status;

enum { BB_GAME_CONNECT4 = 0, BB_GAME_TICTACTOE = 1, BB_GAME_DRAGONCHESS = 2 };
enum { BB_MCTS_DYNAMIC = 0 /* DynamicMCTS.py:14-34 */, BB_MCTS_FIXED = 1 /* FixedMCTS.py:21-34 */ };
enum {
    BB_EVAL_HASH = 0,   /* deterministic synthetic evaluator (validation only; spec in DESIGN.md)  */
    BB_EVAL_NET = 1,    /* Model.SampleValue/GetPriors: residual tower (Blackbird.py:350-389)      */
    BB_EVAL_ROLLOUT = 2 /* MCTS.SampleValue/GetPriors: random rollouts, priors = ones (MCTS.py:346-383) */
};

/* ---- packed game states (the SoA/bit-plane form the engine keeps in HBM) ----------------
 * Connect4 / TicTacToe: 16 bytes, two little-endian u64 bit-planes.
 *   plane p (p=0,1) bit (row*STRIDE + col) = Board[row][col][p]   (Connect4.py:20, TicTacToe.py:19)
 *   STRIDE = 8 for Connect4 (6x7), 4 for TicTacToe (3x3); the spare column is always 0.
 *   plane 0 bits 56-57 = Player (1|2), bits 58-59 = PreviousPlayer (0 = None).
 * DragonChess: 80 bytes: int8 board[64] (row*8+col, signed codes K1 P2 N3 B4 R5 Q6,
 *   DragonChess.py:12-19), int8 player, int8 prev, int8 castle[4] {wK,wQ,bK,bQ}, 10 pad bytes. */
#define BB_GRID_STATE_BYTES 16
#define BB_DC_STATE_BYTES 80

typedef struct {
    int32_t H, W, C;       /* AsInputArray shape [1,H,W,C] */
    int32_t A;             /* LegalMoves */
    int32_t S;             /* child slots per node row, the length of every [n][S] output.  Dense games: >= LegalMoves.
                            * DragonChess (144): the most edges a tree node holds -- a position with more legal moves
                            * (hand-built ones exist) is never expanded: its simulations count in `overflow`, and
                            * bb_sample_moves answers BB_ERR_STATE for a slot whose root it is.  bb_game_* have no bound. */
    int32_t state_bytes;   /* packed state size */
    int32_t dense;         /* 1: slot i == action i; 0: compact child lists (DragonChess) */
    int32_t example_bytes; /* size of one bb_examples_fetch record */
} bb_game_info;

int bb_game_info_get(int game, bb_game_info *out);
/* The number of board symmetries bb_examples_to_batch_sym knows for the game (index 0 is the identity; the others are listed
 * in csrc/symmetry.h): Connect4 2 (the column mirror), TicTacToe 8 (the square's), DragonChess 1.  BB_ERR_ARG: unknown game. */
int bb_game_symmetries(int game);
const char *bb_last_error(void);
int bb_device_count(void);

/* ---- batched game kernels (stateless) ---------------------------------------------------
 * n boards per call, one packed state each; n == 0 is a no-op (BB_OK, nothing touched).      */
/* GameState.LegalActions (Connect4.py:30-36, TicTacToe.py:29-36, DragonChess.py:78-106):
 * legal_out[n][A] bytes 0/1. */
int bb_game_legal(int game, int n, const void *states, uint8_t *legal_out);
/* GameState.ApplyAction (Connect4.py:41-53, TicTacToe.py:41-48, DragonChess.py:127-159 + Move :172-214).
 * states updated in place; status_out[i] = 0, or -1 where the reference raises
 * ValueError('Tried to make an illegal move.') (state left unchanged). */
int bb_game_apply(int game, int n, void *states, const int32_t *actions, int32_t *status_out);
/* GameState.Winner(prevAction) (Connect4.py:62-83, TicTacToe.py:57-76, DragonChess.py:161-167).
 * prev_actions may be NULL (== None for every board); an entry < 0 is None.
 * winner_out[i] = -1 (None), 0 (draw), 1, 2. */
int bb_game_winner(int game, int n, const void *states, const int32_t *prev_actions, int8_t *winner_out);
/* GameState.AsInputArray (Connect4.py:55-60, TicTacToe.py:50-55, DragonChess.py:111-125):
 * planes_out[n][H][W][C] int8. */
int bb_game_encode(int game, int n, const void *states, int8_t *planes_out);
/* initial position (Connect4.py:19-22, TicTacToe.py:18-21, DragonChess.py:36-60) */
int bb_game_initial(int game, void *state_out);

/* ---- network weights: TF variable layout of NetworkFactory.py:37-183 ------ */
typedef struct {
    int32_t H, W, C, F, R, D, A;
    const float *conv0_k;  /* [3][3][C][F]  resTower/conv_block/conv/kernel (HWIO) */
    const float *conv0_b;  /* [F] */
    const float *conv0_bn; /* [4][F] gamma, beta, moving_mean, moving_variance */
    const float *blk_k;    /* [R][2][3][3][F][F]  resTower/block_i/conv_{1,2}/kernel */
    const float *blk_b;    /* [R][2][F] */
    const float *blk_bn;   /* [R][2][4][F] */
    const float *v_conv_k; /* [F]     value/convolution/kernel [1,1,F,1] */
    const float *v_conv_b; /* [1] */
    const float *v_bn;     /* [4][1] */
    const float *v_d1_k;   /* [D]     value/dense_1/kernel [1,D] */
    const float *v_d1_b;   /* [D] */
    const float *v_d2_k;   /* [D]     value/dense_2/kernel [D,1] */
    const float *v_d2_b;   /* [1] */
    const float *p_conv_k; /* [F][2]  policy/convolution/kernel [1,1,F,2] */
    const float *p_conv_b; /* [2] */
    const float *p_bn;     /* [4][2] */
    const float *p_d_k;    /* [2][A]  policy/policy/kernel */
    const float *p_d_b;    /* [A] */
} bb_net_weights;

/* The float blocks of bb_net_weights once more, as a table in the struct's order: X(field, kind, units, floats per unit).  A
 * block is `units` equal pieces back to back; the counts are in terms of the shape fields, which the place that expands the
 * table names C, F, R, D, A.  A kernel unit is one variable of the L2 term, a bias unit one that is not, and a batch-norm unit
 * is [4][n]: its first half (gamma, beta) two trainable variables, its second half (moving mean, variance) constants. */
enum { BB_BLOCK_KERNEL = 0, BB_BLOCK_BIAS = 1, BB_BLOCK_BN = 2 };
#define BB_NET_BLOCKS(X)                          \
    X(conv0_k,  BB_BLOCK_KERNEL, 1,     9 * C * F) \
    X(conv0_b,  BB_BLOCK_BIAS,   1,     F)         \
    X(conv0_bn, BB_BLOCK_BN,     1,     4 * F)     \
    X(blk_k,    BB_BLOCK_KERNEL, 2 * R, 9 * F * F) \
    X(blk_b,    BB_BLOCK_BIAS,   2 * R, F)         \
    X(blk_bn,   BB_BLOCK_BN,     2 * R, 4 * F)     \
    X(v_conv_k, BB_BLOCK_KERNEL, 1,     F)         \
    X(v_conv_b, BB_BLOCK_BIAS,   1,     1)         \
    X(v_bn,     BB_BLOCK_BN,     1,     4 * 1)     \
    X(v_d1_k,   BB_BLOCK_KERNEL, 1,     D)         \
    X(v_d1_b,   BB_BLOCK_BIAS,   1,     D)         \
    X(v_d2_k,   BB_BLOCK_KERNEL, 1,     D)         \
    X(v_d2_b,   BB_BLOCK_BIAS,   1,     1)         \
    X(p_conv_k, BB_BLOCK_KERNEL, 1,     F * 2)     \
    X(p_conv_b, BB_BLOCK_BIAS,   1,     2)         \
    X(p_bn,     BB_BLOCK_BN,     1,     4 * 2)     \
    X(p_d_k,    BB_BLOCK_KERNEL, 1,     2 * A)     \
    X(p_d_b,    BB_BLOCK_BIAS,   1,     A)

/* ---- engine -------------------------------------------------------------------------------- */
typedef struct {
    int32_t game;          /* BB_GAME_* */
    int32_t n_slots;       /* concurrent games (trees) resident on this GPU */
    int32_t mcts_kind;     /* BB_MCTS_* */
    int32_t max_depth;     /* FixedMCTS.MaxDepth (FixedMCTS.py:8-18) */
    int32_t evaluator;     /* BB_EVAL_* */
    int32_t sims_per_move; /* MCTS.PlayLimit (MCTS.py:114-120) */
    int32_t max_plies;     /* cap on game length (Connect4 42, TicTacToe 9; DragonChess has none
                              in the reference -> documented deviation) */
    int32_t max_games;     /* self-play games this engine may store examples for */
    double c_puct;         /* MCTS.ExplorationRate */
    uint64_t seed;         /* Philox key */
    uint64_t hash_salt;    /* BB_EVAL_HASH salt */
    uint32_t first_game_id;/* global index of this engine's game 0 (rank offset; RNG stream id) */
    int32_t noise_on;      /* NetworkFactory.py:176-180 Beta(alpha,1-alpha) prior noise */
    float alpha, epsilon;
    int32_t device;        /* HIP device ordinal */
    int32_t salt_per_game; /* 1: hash salt += local game index (test fixtures) */
    int32_t node_capacity; /* nodes per slot; 0 = sims_per_move*max_plies + 2 */
    int32_t net_form;      /* BB_NET_FORM_*: the arithmetic of the conv tower (Network.getEvaluation/getPolicy, Network.py:48-64).
                              0 = AUTO: the fastest form that meets the 1e-5 bound (the split-operand form wherever it exists) */
    int32_t launch;        /* BB_LAUNCH_*: launch structure of bb_selfplay_step; 0 = AUTO (persistent kernels where the network
                              fits them).  The others exist for parity checks: every structure gives the same bits.
                              BB_LAUNCH_WAVE is the one value that concerns bb_run_sims instead (opt-in, bb_run_sims_structure) */
    int32_t general_net;   /* 1: run a 16-filter network through the launch-per-layer kernels of wider networks (parity checks) */
    int32_t track_ancestors; /* 1: keep, per slot, the chain of edges from the first root to the current one (at most
                              max_plies + 2 of them) and back every simulation up through it, as the reference's _backProp does
                              (MCTS.py:238-258) -- what MCTS.ResetRoot (:214-225) needs.  Every game under bb_run_sims.  Self-play
                              of Connect4 and TicTacToe keeps the chain too, in every launch structure: a slot's chain starts at
                              its game's first position and grows with every move; with a network and BB_LAUNCH_AUTO such an
                              engine plays the asynchronous rounds instead of the persistent kernel, whose backups do not walk
                              the chain (bb_selfplay_mode says 1; the records are the same byte for byte).  DragonChess
                              self-play refuses such an engine (BB_ERR_STATE).  A chain that outgrows its max_plies + 2 entries
                              is marked broken, not cut short: bb_reset_roots */
    int32_t search_cache;  /* 1: bb_run_sims / bb_run_sims_masked probe the engine's evaluation cache before the network, answer hits
                              from it and store misses -- where they search through BB_LAUNCH_WAVE with a network (bb_run_sims_structure)
                              and the game has a cache key (Connect4, DragonChess); the engine then owns a table (sized by
                              BB_EVAL_CACHE_LOG2, none with BB_EVAL_CACHE=0), cleared at every bb_load_weights.  Trees, moves and node rows are
                              unchanged bit for bit; only the evals / eval_cache_* counters differ.  Everywhere else the flag is
                              accepted and nothing is probed.  0 (default): no probe.  Any other value: BB_ERR_ARG */
} bb_config;

/* bb_config.net_form */
#define BB_NET_FORM_AUTO 0
#define BB_NET_FORM_F32 1   /* float32 MFMA (v_mfma_f32_16x16x4_f32): bit-identical to a k-ordered fmaf chain */
#define BB_NET_FORM_SPLIT 2 /* float32 operands as three exact bf16 planes, six bf16 MFMA products per K slice, float32
                               accumulation: float32-grade (<= 1e-5 of the form above, tests/test_gpu_net.py), 2.4x the throughput */
/* bb_config.launch */
#define BB_LAUNCH_AUTO 0
#define BB_LAUNCH_LOCKSTEP 1 /* one tree + one evaluator launch per simulation, one move launch per ply */
#define BB_LAUNCH_ROUNDS 2   /* asynchronous rounds: k_tree_async + a compacted network launch (dense games) */
#define BB_LAUNCH_WAVE 3     /* bb_run_sims / bb_run_sims_masked in ONE launch, one wave per slot (bb_run_sims_structure says where it
                                applies: Connect4, TicTacToe, and DragonChess with a 16-filter network of at most 8 blocks; the
                                rollout evaluator of every game after bb_search_rollouts(e, 1));
                                bb_selfplay_step treats it as BB_LAUNCH_LOCKSTEP.  With bb_config.search_cache that launch also
                                probes the evaluation cache */

typedef struct bb_engine bb_engine;

typedef struct {
    uint64_t sims;            /* simulations completed */
    uint64_t sum_depth;       /* sum over simulations of the leaf depth (edges) */
    uint64_t nodes;           /* tree nodes created */
    uint64_t terminal_leaves; /* simulations that ended on a terminal leaf */
    uint64_t games_finished;
    uint64_t plies;           /* moves played in self-play */
    uint64_t overflow;        /* simulations cut short by pool/path limits (must be 0) */
    uint64_t examples;        /* examples stored */
    uint64_t evals;           /* network tower runs (< sims when known terminal values are reused; evaluation-cache hits not included,
                                 in self-play and in a bb_run_sims that probes alike) */
    uint64_t eval_cache_hits;   /* evaluations served by the evaluation cache: Connect4 self-play in the persistent kernel and in asynchronous rounds (any network, BB_LAUNCH_ROUNDS), one-wave-per-game DragonChess self-play, and the one-launch search (bb_run_sims with BB_LAUNCH_WAVE and bb_config.search_cache); the lock-step search does not probe */
    uint64_t eval_cache_probes; /* evaluations that looked it up: hits + the tower runs among them (a search that probes: probes == evals + hits) */
} bb_counters;

/* bb_create fails with BB_ERR_CAPACITY (before allocating anything) when the pools of cfg->n_slots games -- sized for the
 * worst case: sims_per_move * max_plies nodes per game -- do not fit the device's free memory. */
int bb_create(const bb_config *cfg, bb_engine **out);
/* The largest slot count <= cfg->n_slots whose pools fit the free memory of cfg->device, and the bytes one slot takes.
 * Games are independent and a slot plays game ids g, g+n_slots, ... one after another, so fewer slots change the
 * schedule, never the results.  The reference has no such limit (one Python object graph per game, Blackbird.py:238-251);
 * the batched GenerateTrainingSamples uses this to cap its concurrency.  BB_ERR_CAPACITY if not even one slot fits. */
int bb_fit_slots(const bb_config *cfg, int *n_slots_out, uint64_t *bytes_per_slot_out);
int bb_destroy(bb_engine *e);
/* Network.__init__/loadModel (Network.py:10-28, 100-112): install weights for BB_EVAL_NET.  BB_ERR_ARG, the engine left as it
 * was: a shape that is not the game's or out of range, a null weight block (blk_* may be null where R == 0) */
int bb_load_weights(bb_engine *e, const bb_net_weights *w);
/* bb_load_weights for weights that are in DEVICE memory (on request: nothing calls it unless asked).  w_dev's shape fields are
 * as for bb_load_weights; its pointers are device pointers on the engine's device, which must be the current device, and need to
 * stay valid only until `stream` (a hipStream_t; NULL: the default stream) has run what this call queued on it.  The operand
 * images are packed by kernels (csrc/net_pack.hip.h: the bodies of csrc/net_pack.h, one thread per call) into the buffers the
 * engine's last bb_load_weights made, and are those a bb_load_weights of the same values would upload, byte for byte.
 * Ordering: the kernels run on the engine's stream behind everything `stream` held at the call (an event), after the clearing of
 * the evaluation cache that bb_load_weights does; the engine's other stream and `stream` itself wait for them.  The call waits on
 * the host for the ENGINE's streams first (weights do not change under a running search); it does not synchronise `stream`,
 * copies nothing to the host and allocates nothing.
 * Scope: 16 filters, every game, the fused tower in both net forms (BB_NET_FORM_F32: no bf16 images).  BB_ERR_STATE: an engine
 * that never had bb_load_weights (that call allocates the buffers), one whose loaded shape (C, R, D, A, net form) is not w_dev's,
 * one on the launch-per-layer path (more than 16 filters, bb_config.general_net).  BB_ERR_ARG: a null argument or weight block, a
 * shape that is not the game's, another current device.  Every check comes before any device work; a refused call changes nothing. */
int bb_load_weights_device(bb_engine *e, const bb_net_weights *w_dev, void *stream);
/* Diagnostic: one of the engine's operand buffers copied to the host as it stands (after waiting for the engine's streams) --
 * the float32 first convolution, tower and epilogue records, the head array, or the bf16 images back to back (0 bytes on an
 * engine without them).  *bytes_out (may be NULL) receives the image's size; host_out == NULL: the size only; else capacity, the
 * bytes host_out holds, must cover it (BB_ERR_ARG).  BB_ERR_WEIGHTS before bb_load_weights.  Layouts: csrc/net_pack.h. */
enum { BB_WEIGHTS_W0 = 0, BB_WEIGHTS_WT = 1, BB_WEIGHTS_EPI = 2, BB_WEIGHTS_HEAD = 3, BB_WEIGHTS_X3 = 4 };
int bb_weights_read(bb_engine *e, int which, void *host_out, int64_t capacity, int64_t *bytes_out);
int bb_get_counters(bb_engine *e, bb_counters *out);
int bb_reset_counters(bb_engine *e);
int bb_synchronize(bb_engine *e);
/* MCTS.PlayLimit can be changed between moves (it is a plain attribute, MCTS.py:116-117). */
int bb_set_sims_per_move(bb_engine *e, int sims);
/* Measurement aid: bracket every `every_n`-th evaluator (network) launch with HIP
 * events on the engine's stream; bb_timing_read synchronises, returns mean/min launch duration in
 * milliseconds over the recorded launches and clears the record.  every_n = 0 turns it off. */
int bb_timing_enable(bb_engine *e, int every_n);
int bb_timing_read(bb_engine *e, double *mean_ms_out, double *min_ms_out, int *count_out);
/* Time `iters` back-to-back launches of the network kernel over the n_slots leaf mailbox (HIP events
 * on the engine stream).  ablate != 0 switches parts of the kernel off: only in a diagnostic build (-DBB_DIAG; kernel tuning,
 * results are wrong) -- the product library has no such switches and answers BB_ERR_ARG. */
int bb_timing_net(bb_engine *e, int iters, int noise, int ablate, double *ms_per_launch_out);
/* Which launch structure bb_selfplay_step uses: 0 lock-step (one tree + one evaluator launch per
 * simulation), 1 asynchronous rounds, 3 persistent per-CU kernel with a work queue between its tree and network
 * waves (default for networks that fit LDS), 5 DragonChess with the 16-filter network: one wave keeps its game for a
 * whole launch -- tree step, network and move in the same wave, 6 the rollout evaluator after bb_selfplay_rollouts(e, 1): one
 * launch per bb_selfplay_step, one wave per slot -- tree step, playout, move and slot refill in the same wave.  (2 and 4 were
 * launch structures that measured slower and were retired.) */
int bb_selfplay_mode(bb_engine *e);
/* Opt-in for BB_EVAL_ROLLOUT engines (MCTS.SampleValue, MCTS.py:360-383: FixedMCTS, plain DynamicMCTS), called after bb_create:
 * on = 1 lets bb_selfplay_step play in one launch per call instead of sims_per_move x 2 + 1 launches per ply -- the wave of a
 * slot does tree descent, playout, backup, move, example record and slot refill, for every game and both mcts_kinds, whatever
 * bb_config.launch says.  Every slot makes exactly `plies` moves per call, and records, headers, counters and random streams are
 * the lock-step ones byte for byte (the draws are keyed by game id, simulation serial and step, not by who computes them).  A
 * call of many or long plies is cut into several launches on the host, which changes no result.  on = 0 (the state after
 * bb_create): lock-step.  bb_selfplay_mode reports the result.  Independent of bb_search_rollouts (below), which concerns
 * bb_run_sims only.  On an engine with another evaluator the call is accepted and changes nothing.  BB_ERR_ARG: null engine, or
 * `on` other than 0 / 1. */
int bb_selfplay_rollouts(bb_engine *e, int on);
/* Which arithmetic the loaded network's conv tower runs in (after bb_load_weights): 0 float32 MFMA, fused 16-filter
 * tower (bit-identical to the k-ordered fmaf chain); 1 float32 MFMA, one launch per conv layer (any multiple of 16
 * filters); 2 float32 results on the bf16 matrix pipe -- every operand split exactly into three bf16 values, six MFMA
 * products per K slice, float32 accumulation (every 16-filter network: Connect4, TicTacToe and DragonChess; 1e-5 of form 0, not
 * bit-identical; bb_config.net_form = BB_NET_FORM_F32 selects form 0 instead); 3 the launch-per-layer network with its tower
 * layers in the split-operand form of 2 (BB_NET_FORM_F32: form 1).  Negative: BB_ERR_*. */
int bb_net_form(bb_engine *e);
/* How a bb_net_eval / bb_net_eval_keyed call of n positions is cut into launches by the engine as it stands (after
 * bb_load_weights): *out = BB_NET_EVAL_FUSED (bb_net_form 0 / 2), or, for the launch-per-layer network (bb_net_form 1 / 3),
 * BB_NET_EVAL_SMALL (one position x one filter block per wave: the latency of few positions) or BB_NET_EVAL_BATCH (several
 * positions x several filter blocks per wave: throughput).  Both give the same bits; self-play rounds, whose batch size lives
 * on the device, always take BB_NET_EVAL_BATCH.  Launches nothing.  BB_ERR_ARG: a null argument or n < 0; BB_ERR_WEIGHTS:
 * before bb_load_weights. */
#define BB_NET_EVAL_FUSED 0
#define BB_NET_EVAL_SMALL 1
#define BB_NET_EVAL_BATCH 2
int bb_net_eval_structure(bb_engine *e, int n, int32_t *out);

/* Network.getEvaluation + getPolicy for n positions (Network.py:48-64; graph NetworkFactory.py:22-183).
 * Exactly one of states (packed) / planes (int8 [n][H][W][C], what AsInputArray returns) is non-NULL.
 * value_out[n] tanh value for the side to move; logits_out[n][A] pre-softmax; policy_out[n][A]
 * softmax, mixed with Beta noise and re-normalised when noise != 0 (the value of `noise` selects the
 * random stream, so successive calls can draw fresh noise like successive sess.run calls do).
 * Outputs may be NULL. */
int bb_net_eval(bb_engine *e, int n, const void *states, const int8_t *planes, float *value_out,
                float *logits_out, float *policy_out, int noise);
/* The same forward pass with the prior-noise stream named explicitly: position i draws the Beta(alpha, 1-alpha) noise
 * of (global game id game_ids[i], node serial node_serials[i]) -- the key the self-play kernels use for the node they
 * expand -- so a checker can obtain exactly the priors the engine used inside a search
 * (Model.GetPriors with the graph's noise, Blackbird.py:372-389 + NetworkFactory.py:176-182). */
int bb_net_eval_keyed(bb_engine *e, int n, const void *states, const int8_t *planes, const uint32_t *game_ids,
                      const int32_t *node_serials, float *value_out, float *logits_out, float *policy_out);
/* the validation evaluator, same outputs (policy unnormalised, as getPolicy-shaped input to GetPriors) */
int bb_hash_eval(bb_engine *e, int n, const void *states, float *value_out, float *policy_out);

/* ---- tree search on resident slots (MCTS.FindMove split into its steps) ---------------------- */
/* DropRoot (MCTS.py:141-144) + prime slot i's root with states[i] (FindMove's `Root is None`
 * branch, MCTS.py:184-186).  game_ids may be NULL. */
int bb_set_roots(bb_engine *e, int n, const int32_t *slots, const void *states, const uint32_t *game_ids);
/* _runMCTS (MCTS.py:284-303): `sims` more simulations on every active slot, playLimit semantics
 * (added to Root.Plays). */
int bb_run_sims(bb_engine *e, int sims);
/* The same for the slots with mask[slot] != 0 only (mask[n_slots], host memory); the other slots' trees are left
 * untouched.  This is what a batched arena needs (Blackbird.py:177-216, TestModels: two searchers share the games and
 * each one only searches the positions where it is to move). */
int bb_run_sims_masked(bb_engine *e, int sims, const uint8_t *mask);
/* Which launch structure bb_run_sims / bb_run_sims_masked use for this engine as it stands: *out = BB_LAUNCH_LOCKSTEP (one tree
 * + one evaluator launch per simulation of _runMCTS, MCTS.py:284-303) or BB_LAUNCH_WAVE (one launch per call: a wave keeps its
 * slot and runs _findLeaf / the evaluator / _backProp, MCTS.py:238-258, 305-334, for its own leaf, simulation after
 * simulation -- the same trees bit for bit).  BB_LAUNCH_WAVE is what an engine created with bb_config.launch = BB_LAUNCH_WAVE
 * gets when its evaluator is BB_EVAL_NET with a 16-filter network in the split-operand form (bb_net_form 2) -- for DragonChess
 * one of at most 8 residual blocks, what its kernel keeps in LDS -- or when its game is Connect4 or TicTacToe and its evaluator
 * is BB_EVAL_HASH, or when its evaluator is BB_EVAL_ROLLOUT and bb_search_rollouts(e, 1) was called; every other engine (DragonChess
 * with BB_EVAL_HASH or a deeper tower, rollouts without that call, wide networks, BB_NET_FORM_F32, general_net) searches lock-step whatever it asked for, and says so here.  Read it after bb_load_weights: a network evaluator
 * without weights answers BB_ERR_WEIGHTS. */
int bb_run_sims_structure(bb_engine *e, int32_t *out);
/* Opt-in for BB_EVAL_ROLLOUT engines (MCTS.SampleValue, MCTS.py:360-383: FixedMCTS, plain DynamicMCTS), called after bb_create:
 * on = 1 lets an engine created with bb_config.launch = BB_LAUNCH_WAVE search through BB_LAUNCH_WAVE as well -- tree descent, the
 * random playout of the leaf and the backup in the slot's own wave, every game and both mcts_kinds, the same trees bit for bit
 * (the playout's draws are keyed by game id, simulation serial and step, not by who computes them).  on = 0 (the state after
 * bb_create): such an engine searches lock-step.  bb_run_sims_structure reports the result.  On an engine with another evaluator or
 * another launch value the call is accepted and changes nothing; self-play is not concerned (bb_selfplay_rollouts).  BB_ERR_ARG: null engine, or `on`
 * other than 0 / 1. */
int bb_search_rollouts(bb_engine *e, int on);
/* After bb_run_sims: Root statistics + the move _selectAction(exploring=False) picks (MCTS.py:335-338).
 * u[n_slots] uniforms in [0,1) for np.random.choice's law, or NULL to draw Philox(seed, game_id, ply).
 * Outputs per slot (S = bb_game_info.S): action (or BB_ERR_NAN), root_winrate = Root.WinRate(),
 * root_plays, child_action[S] (-1 pad), child_plays[S], child_value[S] (Node.Value of the child, f32).
 * Any output pointer may be NULL.  action is BB_ERR_NAN where sum(N ^ (1 / temp)) is not a positive finite number: 0 / 0, or inf / inf
 * when a power overflows (np.random.choice raises ValueError there). */
int bb_sample_moves(bb_engine *e, double temp, const double *u, int32_t *action_out,
                    float *root_winrate_out, int32_t *root_plays_out, int32_t *child_action_out,
                    int32_t *child_plays_out, float *child_value_out);
/* MoveRoot (MCTS.py:201-212, 260-282) by action id; actions[i] < 0 leaves slot i alone. */
int bb_move_roots(bb_engine *e, const int32_t *actions);
int bb_get_root_states(bb_engine *e, void *states_out);
/* MCTS.ResetRoot (MCTS.py:214-225): every slot's root goes back to its top-most ancestor (the first position searched) with all
 * statistics intact, including the simulations run from the positions below it (bb_config.track_ancestors; BB_ERR_STATE otherwise).
 * A tree that restarted since (bb_set_roots, a move from an unexpanded root, a full node pool) starts its chain anew: its root
 * stays.  After bb_selfplay_step a slot's top is the first position of the game it is playing (a slot that went on to its next
 * game: that game's), and its play resumes from there: a simulation that was in flight (the asynchronous rounds stop with one
 * in most slots) is backed up from the new root down, and the slot's ply counter is not wound back, so the records it writes from
 * then on are not a game's -- a look at the tree, not a way to replay.  BB_ERR_CAPACITY, in every game, if a slot moved its root more than
 * max_plies + 2 times since its chain began: its chain is broken -- simulations since then were not backed up above the root, and
 * no later move mends it -- so nothing is changed for any slot; bb_set_roots, bb_selfplay_begin or a restart of the slot's tree
 * starts a whole chain again.  (Self-play ends a game at max_plies moves, so only bb_move_roots can break a chain.) */
int bb_reset_roots(bb_engine *e);
/* One node of a slot's tree, for a host-side Node view (MCTS.py:7-98: Children, Plays, Value, State): node < 0 = the root, else a pool
 * index taken from an earlier view.  child_node_out / child_plays_out / child_value_out [S]: per child slot the child's pool index (-1:
 * no simulation has reached it yet -- the reference's eager AddChildren would hold a Node with zero statistics there when the move is
 * legal), its Plays and Value; state_out: the node's packed state; info_out[3]: flags (bit 0: expanded, bit 1: terminal), legal mask,
 * the node's own pool index.  Dense-action games (a node of every game: bb_node_edges). */
int bb_node_view(bb_engine *e, int slot, int node, int32_t *child_node_out, int32_t *child_plays_out, float *child_value_out,
                 void *state_out, int32_t *info_out);
/* The same node as a list of its children, for every game: node < 0 = the root, else a pool index from an earlier call (BB_ERR_ARG
 * if the slot's tree has no such node).  Every output array has [S] entries; entry k: the child's action id (-1: no child), its pool
 * index (-1 where no simulation has reached it), Plays and Value.  DragonChess lists the node's legal moves in its edge order
 * (the order of bb_sample_moves' child_action_out); the dense games put action i at entry i, -1 at the illegal ones.
 * state_out: the node's packed state; info_out[3]: flags (as bb_node_view), number of children (0 until expanded), pool index. */
int bb_node_edges(bb_engine *e, int slot, int node, int32_t *child_action_out, int32_t *child_node_out, int32_t *child_plays_out,
                  float *child_value_out, void *state_out, int32_t *info_out);

/* Re-key the engine's random streams (Philox key `seed`; global id of local game 0).  The reference draws fresh numpy /
 * TensorFlow randomness on every GenerateTrainingSamples call (MCTS.py:336-338, NetworkFactory.py:176-180); a caller
 * that reuses an engine for another self-play run gives it a new stream here, otherwise the run repeats the last one. */
int bb_set_rng_stream(bb_engine *e, uint64_t seed, uint32_t first_game_id);

/* ---- batched self-play: Blackbird.GenerateTrainingSamples (Blackbird.py:219-268) ------------- */
/* Start `n_games` games (local ids 0..n_games-1; slot g plays ids g, g+n_slots, ...).  A slot whose move has no probabilities
 * (bb_sample_moves' BB_ERR_NAN rule, e.g. N ^ (1 / temp) overflows) stops without a record and counts in bb_counters.overflow. */
int bb_selfplay_begin(bb_engine *e, int n_games, double temp);
/* Start positions for self-play -- an extension: the reference starts every game from `model.Game()` (Blackbird.py:238-251).
 * states: HOST memory, n packed states of the engine's game (the layout and state_bytes of bb_set_roots).  The engine copies the
 * table to the device and owns the copy until the next call or bb_destroy.  In every later bb_selfplay_begin the game with
 * engine-local index k (0 <= k < n_games; game id first_game_id + k) starts from states[k % n], whichever slot plays it and
 * whichever launch structure the engine uses.  Plies count from the start position: the game's first record holds states[k % n]
 * at ply 0, and max_plies caps the plies played from there.  Records keep their layout and the random streams their keys (move
 * draw: seed, game id, ply; prior noise: game id, node serial; playouts as before).
 * n == 0 clears the table (states is ignored): games start from the initial position again.  An engine that never had a table,
 * or has none now, plays exactly as before.
 * Every state is checked on the device before the table is swapped.  BB_ERR_ARG, with the first offending index and the reason
 * in bb_last_error, when (1) the game is already over there (Winner() is not None), (2) it has no legal move, or (3) DragonChess:
 * it has more than S = 144 legal moves (such a root is never expanded); the previous table then stays in force.  Anything else
 * bb_set_roots accepts is accepted: unreachable boards, a DragonChess state in the middle of White's double move.
 * BB_ERR_ARG before any device call: n < 0, states == NULL with n > 0, a null engine.  BB_ERR_CAPACITY: the copy does not fit.
 * For use BETWEEN runs only: the call waits for everything the engine has queued before it swaps the table; calling it while
 * a run started by bb_selfplay_begin is unfinished is not supported (slots refilled later would start from the new table). */
int bb_selfplay_set_starts(bb_engine *e, int n, const void *states);
/* A temperature schedule by ply for self-play -- an extension: the reference plays a whole game at one temperature.  The move out
 * of a position whose record carries ply p is drawn at bb_selfplay_begin's `temp` when p < plies and at temp_late otherwise.  p is
 * the engine's own ply counter, the value in the record header and in the key of the move's draw: ply counts from the game's start
 * position -- 0 for every game, also for one that starts from a bb_selfplay_set_starts state, and 0 again when a slot is refilled
 * with its next game.  temp_late == 0 is the PUCT arg-max move, exactly as temp == 0.  Nothing else about a move changes: the
 * draw of (seed, game id, ply), the record, the re-rooting, and the rule that a move without probabilities (N ^ (1 / temp_late)
 * overflows) stops the slot without a record and counts in bb_counters.overflow.  Every launch structure honours it.
 * plies < 0 turns the schedule off; plies == 0 plays every move at temp_late.  An engine that never had a schedule, has it turned
 * off, or has temp_late == temp plays exactly as without this call.
 * Host state only: it takes effect at the next bb_selfplay_begin, which refuses (BB_ERR_NAN) an engine with fewer than 2
 * simulations per move when EITHER temperature is non-zero.  BB_ERR_ARG: a null engine, temp_late negative or not finite. */
int bb_selfplay_set_temp_schedule(bb_engine *e, int plies, double temp_late);
/* Advance the self-play by `plies` moves' worth of search per active slot (a move: sims_per_move simulations, sample, record
 * the example, MoveRoot, Winner(); finished games hand their slot to the next game id).  Asynchronous.  In the lock-step and
 * rounds structures every slot makes exactly `plies` moves.  The persistent kernels hand out plies x sims_per_move tree visits
 * per slot instead: 7/8 of them go to the slots of each workgroup up front, the rest is one launch-wide pool the workgroups
 * draw from until it is dry -- so every slot advances, by about `plies` moves, a slot in a quicker workgroup by a few more
 * (a game's results do not depend on when its visits happen). */
int bb_selfplay_step(bb_engine *e, int plies);
/* 1 when every game started by bb_selfplay_begin has finished */
int bb_selfplay_done(bb_engine *e, int *done_out, int *games_finished_out);
/* Finished games' examples, in (game, ply) order.  record layout (little endian):
 *   u32 game_id, u16 ply, u8 player, i8 z, u32 total_visits, u32 n_children,
 *   packed state [state_bytes], u32 visits[S], (compact games only) u16 action[S]
 * The last record of a game is the terminal example (visits all zero, Blackbird.py:256-258).
 * Returns the number of records written (<= max_records), or a negative status. */
int bb_examples_fetch(bb_engine *e, int first_game, int n_games, void *records_out, int max_records,
                      int32_t *game_offsets_out /* n_games+1 */, int8_t *winner_out /* n_games */);
/* The [n_games][4] header words of games first_game ..: (n_examples, winner, plies, done).  What GenerateTrainingSamples needs
 * to hand finished games to Conn.PutGames (Blackbird.py:266-268) while the others still play. */
int bb_selfplay_headers(bb_engine *e, int first_game, int n_games, int32_t *hdr_out);
/* bb_examples_fetch for a LIST of games (any order): their records are compacted on the device and come back in one copy.
 * game_offsets_out[n + 1], winner_out[n] as in bb_examples_fetch; a game that has not finished contributes no records. */
int bb_examples_fetch_games(bb_engine *e, int n, const int32_t *game_ids, void *records_out, int max_records,
                            int32_t *game_offsets_out, int8_t *winner_out);
/* The example store where it lives, for a device-to-device exchange (the epoch-end RCCL all-gather of (s, pi, z),
 * SURVEY.md 8e): records_out = device pointer to [max_games][max_plies+1] records of record_bytes each (layout above),
 * game_hdr_out = device pointer to int32 [max_games][4] = {n_examples, winner, plies, done}; game g's records are the
 * first n_examples of its row once done != 0.  Valid until bb_destroy; synchronise (bb_synchronize) before reading. */
int bb_examples_device(bb_engine *e, void **records_out, uint64_t *bytes_out, uint64_t *record_bytes_out,
                       int32_t **game_hdr_out);

/* ---- the arena on the device: Blackbird.TestModels (Blackbird.py:177-216) without the host in the loop ------------ */
/* An arena plays n_games head-to-head games between two engines, `a` (model1) and `b` (model2), one game per slot index, and keeps
 * per game the packed state, whose turn it is, the result and a move log on the device.  A ply of a live game is the reference's
 * loop body: the mover -- a and b alternate every ply whatever state.Player says (Blackbird.py:196-201), DragonChess's W, W, B
 * order included -- primes its slot on its first turn (DropRoot + FindMove's `Root is None` branch, MCTS.py:141-144, 184-186, game
 * id = the slot index), runs its engine's sims_per_move simulations on that slot alone through the structure
 * bb_run_sims_structure reports (_runMCTS, MCTS.py:284-303), picks the move as bb_sample_moves(e, temp, u = NULL) does
 * (_selectAction, MCTS.py:335-338; the Philox draw of (engine seed, game id, ply) when temp != 0), the move is applied, every
 * primed side follows with MoveRoot (Blackbird.py:198-200) and Winner() is asked with no previous action (Blackbird.py:202).  The
 * other side's slot, and every slot of a finished game, is not touched.  Trees, counters and results are those of the same
 * sequence made through bb_set_roots / bb_run_sims_masked / bb_sample_moves / bb_move_roots, bit for bit.
 * Both sides' searches of one ply are enqueued on their engines' own streams and joined with events before the move, so they may
 * overlap; nothing is allocated and nothing waits on the host between plies.
 * The engines are BORROWED: they must outlive the arena, and between bb_arena_begin and the last bb_arena_fetch of a run calling
 * the search or self-play entry points on them (bb_set_roots, bb_run_sims*, bb_sample_moves, bb_move_roots, bb_selfplay_*) is not
 * supported.  bb_get_counters, bb_node_view / bb_node_edges and bb_get_root_states after a bb_arena_status are fine. */
typedef struct bb_arena bb_arena;
/* log_plies: moves logged per game (later moves are played, not logged).  BB_ERR_ARG, before any device call: a null pointer,
 * a == b, engines of different games, n_slots or devices, log_plies < 0. */
int bb_arena_create(bb_engine *a, bb_engine *b, int log_plies, bb_arena **out);
/* Start n_games games (1 <= n_games <= n_slots; the slots beyond stay idle).  a_first[n_games] (host memory, required): a moves
 * first in game i, the coin of Blackbird.py:187-193.  start_states: host memory, n_games packed states, or NULL for `Game()`
 * (Blackbird.py:191); checked as bb_selfplay_set_starts checks its table -- BB_ERR_ARG naming the first index whose game is
 * already over, has no legal move or (DragonChess) more than S legal moves.  temp >= 0 (TestModels' temp, handed to FindMove).
 * Both engines' slots count as unprimed again: DropRoot at the top of every game (Blackbird.py:189-190).  Waits for both engines.
 * BB_ERR_WEIGHTS: a network engine without weights.  BB_ERR_ARG: an engine with fewer than 2 simulations per move and
 * temp != 0 (MCTS.py:336-338, the rule of bb_selfplay_begin), or any argument outside the above. */
int bb_arena_begin(bb_arena *ar, int n_games, const uint8_t *a_first, const void *start_states, double temp);
/* bb_selfplay_set_temp_schedule for the arena: ply p of the match (0 for each game's first move -- ply counts from the game's
 * start position, given or initial; every live game is on the same ply) is sampled as bb_sample_moves(e, p < plies ? temp :
 * temp_late, u = NULL) does.  Call it before bb_arena_begin: a run keeps the schedule it began with.  plies < 0 turns it off.  With
 * a schedule on, bb_arena_begin's rule about fewer than 2 simulations per move looks at both temperatures.
 * BB_ERR_ARG: a null arena, temp_late negative or not finite. */
int bb_arena_set_temp_schedule(bb_arena *ar, int plies, double temp_late);
/* Enqueue `plies` plies of every live game (Blackbird.py:195-203).  Asynchronous: no host synchronisation inside or between the
 * plies; a finished game costs masked-out lanes only. */
int bb_arena_step(bb_arena *ar, int plies);
/* Wait for both engines; *alive_out = games still running.  BB_ERR_CAPACITY if either engine's overflow counter is non-zero (a
 * search tree outgrew its node pool), BB_ERR_NAN if a game stopped on a negative action ('probabilities contain NaN',
 * MCTS.py:336-338) or an illegal move, else BB_OK. */
int bb_arena_status(bb_arena *ar, int *alive_out);
/* result_out[n_games]: +1 / 0 / -1 for a's win / draw / loss (Blackbird.py:204-212; 0 while the game runs); plies_out[n_games]:
 * moves made; moves_out[n_games][log_plies]: the actions, -1 padded; states_out: n_games packed current states.  Any output may
 * be NULL.  Waits for both engines, so it also works in the middle of a run. */
int bb_arena_fetch(bb_arena *ar, int8_t *result_out, int32_t *plies_out, int32_t *moves_out, void *states_out);
/* Waits for both engines and frees the arena's own memory; the engines stay.  NULL: BB_OK. */
int bb_arena_destroy(bb_arena *ar);

/* ---- training batches from example records, on the device ------------------------------------ */
/* What TrainWithExamples stacks per batch (Blackbird.py:300-308: AsInputArray planes, the MCTS policy, z), after the float32
 * conversion of the loss's inputs -- formed where the records are, with nothing staged through the host.  Stateless; ALL
 * pointers are device memory of the calling thread's current device, and the launch is asynchronous on `stream` (a hipStream_t;
 * 0 = the default stream).
 *   records  [n_records][example_bytes], the bb_examples_fetch layout: the engine's own store (bb_examples_device), a compacted
 *            copy or an all-gathered tensor.  16-byte aligned.
 *   index    [n] record of every batch row, in output order; NULL = records 0..n-1.
 * Row k, from record r = records[index[k]] (any single output may be NULL, not all three):
 *   boards_out[k][H][W][C] float32: the AsInputArray planes of r's state (bb_game_encode's values);
 *   policy_out[k][A]       float32: (float)((double)visits_a / (double)total) -- divided in double, rounded once --, all zeros
 *                          when total == 0 (the terminal example).  Dense games: entry a from visits[a], a < A (the spare
 *                          slots A..S-1 are ignored); DragonChess: zeros except entry action[j] from visits[j], j < n_children;
 *   value_out[k]           float32: r.z.
 *   boards_out and policy_out 16-byte aligned.
 * A row is written as all zeros, and *bad_out (when non-NULL) incremented by one per such row, if index[k] is outside
 * [0, n_records), if n_children > S, or if a compact action[j] >= A: malformed input never becomes an out-of-bounds access.
 * n == 0: BB_OK, nothing touched (GPU or not).  n < 0, records NULL, every output NULL, a misaligned pointer: BB_ERR_ARG. */
int bb_examples_to_batch(int game, int n_records, const void *records, int n, const int64_t *index, float *boards_out,
                         float *policy_out, float *value_out, int32_t *bad_out, void *stream);
/* The same batch with every row in an orientation of its own -- an extension (the reference does not augment its examples), opt-in
 * and exact.  bb_examples_to_batch is this call with sym == NULL.  Stateless; ALL pointers are device memory of the calling
 * thread's current device, and the launch is asynchronous on `stream` (a hipStream_t; 0 = the default stream).
 *   records  [n_records][example_bytes], the bb_examples_fetch layout: the engine's own store (bb_examples_device), a compacted
 *            copy or an all-gathered tensor.  16-byte aligned.
 *   index    [n] record of every batch row, in output order; NULL = records 0..n-1.
 *   sym      [n] uint8, the symmetry of every batch row, each < bb_game_symmetries(game) (0 = the identity; the order of the
 *            others, their cell maps and the action maps the rules imply: csrc/symmetry.h); NULL = the identity everywhere.
 * Row k, from record r = records[index[k]] and sigma = sym[k] (any single output may be NULL, not all three):
 *   boards_out[k][H][W][C] float32: the AsInputArray planes of the position r's state becomes under sigma: cell sigma(row, col)
 *                          holds what bb_game_encode gives for cell (row, col) of r's state (the side-to-move plane is constant);
 *   policy_out[k][A]       float32: entry sigma(a) is (float)((double)visits_a / (double)total) -- divided in double, rounded
 *                          once --, all zeros when total == 0 (the terminal example).  Dense games: from visits[a], a < A (the
 *                          spare slots A..S-1 are ignored); DragonChess (sigma is the identity): zeros except entry action[j]
 *                          from visits[j], j < n_children;
 *   value_out[k]           float32: r.z.
 *   boards_out and policy_out 16-byte aligned.
 * A row is written as all zeros, and *bad_out (when non-NULL) incremented by one per such row, if index[k] is outside
 * [0, n_records), if sym[k] >= bb_game_symmetries(game) (DragonChess: anything but 0), if n_children > S, or if a compact
 * action[j] >= A: malformed input never becomes an out-of-bounds access, and a sym[k] out of range never becomes an index.
 * n == 0: BB_OK, nothing touched (GPU or not).  n < 0, records NULL, every output NULL, a misaligned pointer: BB_ERR_ARG. */
int bb_examples_to_batch_sym(int game, int n_records, const void *records, int n, const int64_t *index, const uint8_t *sym,
                             float *boards_out, float *policy_out, float *value_out, int32_t *bad_out, void *stream);

/* ---- duplicate positions merged into one training row (Connect4, TicTacToe) -------------------- */
/* An extension (the reference trains on every stored row), opt-in.  Concurrent self-play from one start position stores the same
 * position many times, each copy with its own visit counts and outcome; bb_examples_merge groups the records by position and sums
 * their targets, bb_examples_merged_to_batch forms training rows from the sums.  Definition:
 *   key      what the network sees of a record's state: the cells of both players and the side to move.  The previous player,
 *            game_id, ply and player of the header are not part of it.  Equal keys: the same position.
 *   groups   numbered 0 .. n_groups-1 by the index of their first member in record order: rep[] is ascending.  A record with
 *            n_children > S belongs to no group: group -1, one count in *bad_out, and nothing it says is used as an address.
 *   sums     count[g] (int32), zsum[g] (int32, of z), total[g] (uint64, of total), visits[g][a], a < A (uint64, of visits[a]).
 *   row      planes of record rep[g]; policy[a] = (float)((double)visits[g][a] / (double)total[g]), zeros when total[g] == 0;
 *            value = (float)((double)zsum[g] / (double)count[g]).  The policy pools visits: a copy searched longer weighs more.
 *            A group of one member is, bit for bit, that record's row of bb_examples_to_batch.
 * All sums are integers and no float atomic is used: the same input gives the same bits on every run.
 * DragonChess, an unknown game, n_records < 0 or a null or misaligned pointer: BB_ERR_ARG before any device call.  Stateless; ALL
 * pointers but bytes_out are device memory of the calling thread's current device; the launches are asynchronous on `stream`,
 * nothing is allocated and nothing is waited for. */
/* The scratch memory bb_examples_merge needs for n_records records, in bytes (0 for none).  Host only: no device call. */
int bb_examples_merge_workspace(int game, int n_records, uint64_t *bytes_out);
/*   records     [n_records][example_bytes], the bb_examples_fetch layout, 16-byte aligned; read only
 *   group_out   [n_records] the group of every record, -1 for a malformed one
 *   rep_out, count_out, zsum_out, total_out [n_records], visits_out [n_records][A]: entries 0 .. n_groups-1 are written
 *   n_groups_out  [1] the number of groups -- or BB_ERR_CAPACITY if a probe of the position table ran its whole (bounded) length
 *                 without finding a place, which a table of twice the records cannot do unless memory was damaged: the caller's
 *                 one look at this word after the stream has run is where that is reported, and no other output is valid then
 *   bad_out     [1] incremented by one per malformed record (the caller zeroes it)
 *   workspace   workspace_bytes >= bb_examples_merge_workspace bytes, 16-byte aligned; contents need not be kept
 * n_records == 0: BB_OK, nothing touched (GPU or not). */
int bb_examples_merge(int game, int n_records, const void *records, int32_t *group_out, int32_t *rep_out, int32_t *count_out,
                      int32_t *zsum_out, uint64_t *total_out, uint64_t *visits_out, int32_t *n_groups_out, int32_t *bad_out,
                      void *workspace, uint64_t workspace_bytes, void *stream);
/* bb_examples_to_batch_sym over merged rows: row k is group index[k] (NULL: group k; n rows) in the orientation sym[k] (NULL: as
 * played), from rep / count / zsum / total / visits as bb_examples_merge filled them for these records (n_groups the host's copy of
 * its count).  Outputs, alignment and the n == 0 rule as there.  A row is zeros, and *bad_out incremented, if index[k] is outside
 * [0, n_groups), if sym[k] >= bb_game_symmetries(game), if rep is outside [0, n_records) or names a malformed record, or if count is
 * not positive: no value becomes an index before it has been checked. */
int bb_examples_merged_to_batch(int game, int n_records, const void *records, int n_groups, const int32_t *rep, const int32_t *count,
                                const int32_t *zsum, const uint64_t *total, const uint64_t *visits, int n, const int64_t *index,
                                const uint8_t *sym, float *boards_out, float *policy_out, float *value_out, int32_t *bad_out,
                                void *stream);

/* ---- the training step as HIP kernels (opt-in; the default trainer is PyTorch's autograd) --------- */
/* One step of Network.train (Network.py:66-84; loss and optimiser NetworkFactory.py:185-245) for the dense games (Connect4,
 * TicTacToe) with 16 filters, 0..9 blocks and a dense width of 1..64: three launches (csrc/train.hip.h) -- the step's noise,
 * label sum and L2 term; one workgroup per example (forward, loss pieces, backward, the gradients of every trainable variable
 * into the example's own slab); per parameter element the slabs summed in example order, + v / N for the non-bias variables,
 * and the TF1 update (Adam with epsilon outside the bias correction, Momentum, GradientDescent) in place.  No float atomics:
 * the same steps give the same bits.  Batch norm is in inference mode: the moving statistics are constants.
 * DragonChess (17 planes, 4032 actions) is covered too, with 16 filters, a dense width of 1..64 and 0..8 blocks -- the most whose
 * per-example workgroup fits the 160 KB of LDS of a CU; bb_trainer_create's refusal names the figure.  Such a trainer steps from
 * batch tensors only: bb_trainer_step, bb_trainer_read (BB_TRAIN_NOISE: 4032 floats), bb_trainer_param_count,
 * bb_trainer_load_engine and bb_trainer_destroy work for it; bb_trainer_epoch, bb_trainer_eval and bb_trainer_eval_tensors
 * return BB_ERR_ARG (a DragonChess record holds a compact child list: the records source and the scorer do not cover it). */
enum { BB_OPT_ADAM = 0, BB_OPT_MOMENTUM = 1, BB_OPT_SGD = 2 };
enum { BB_TRAIN_PARAMS = 0, BB_TRAIN_GRADS = 1, BB_TRAIN_SLOT_M = 2, BB_TRAIN_SLOT_V = 3, BB_TRAIN_NOISE = 4 };
typedef struct {
    int32_t game;      /* BB_GAME_CONNECT4 | BB_GAME_TICTACTOE | BB_GAME_DRAGONCHESS */
    int32_t optimizer; /* BB_OPT_* */
    int32_t max_batch; /* examples per step at most: one gradient slab each is allocated */
    int32_t device;    /* HIP device ordinal */
    float momentum;    /* BB_OPT_MOMENTUM */
    float alpha, epsilon; /* the graph's Beta(alpha, 1-alpha) noise and its weight (NetworkFactory.py:176-182); epsilon 0: none */
    uint64_t seed;     /* Philox key of the noise drawn on the device; the counter is the number of steps made so far */
} bb_train_config;
typedef struct bb_trainer bb_trainer;
/* w: the initial weights (host or device memory).  BB_ERR_ARG for a game, a shape, an optimiser or a max_batch outside the scope
 * above -- checked before any device call; BB_ERR_HIP without a GPU; BB_ERR_CAPACITY if the slabs do not fit the free memory. */
int bb_trainer_create(const bb_train_config *cfg, const bb_net_weights *w, bb_trainer **out);
int bb_trainer_destroy(bb_trainer *t);
/* The loss of the steps made after this call (an extension; a trainer is created with BB_LOSS_REFERENCE, the reference graph's
 * loss described above, and behaves bit for bit as before until this is called).  BB_LOSS_PER_EXAMPLE, for a batch of n rows with
 * value v_b, logits lg_b, policy label pi_b and outcome z_b:
 *   lossEvaluation = (1/n) sum_b (v_b - z_b)^2                                  (as the reference's)
 *   lossPolicy     = -(1/n) sum_b sum_a pi_b[a] log_softmax(lg_b)[a]            a row whose label is all zeros adds 0
 *   lossParam      = l2 * sum over the trainable non-bias variables of sum(v^2)/2
 *   d loss / d lg_b[a] = (softmax_b[a] T_b - pi_b[a]) / n, T_b = sum_a pi_b[a];  d lossParam / d v = l2 * v
 * No noise: alpha and epsilon are not used, nothing is drawn (BB_TRAIN_NOISE reads zeros), and bb_trainer_step / bb_trainer_epoch
 * return BB_ERR_ARG for a noise pointer.  The same three launches with the loss as a compile-time argument of the kernels
 * (csrc/train.hip.h), no float atomics: the same steps give the same bits.  l2 is read with BB_LOSS_PER_EXAMPLE only.  Host state
 * alone: callable at any time between steps, no device call, no allocation; optimiser slots and step counts carry over.
 * BB_ERR_ARG: an unknown loss, an l2 that is negative or not finite (as a float32 too), a null trainer. */
enum { BB_LOSS_REFERENCE = 0, BB_LOSS_PER_EXAMPLE = 1 };
int bb_trainer_set_loss(bb_trainer *t, int loss, double l2);
/* boards [n][H][W][C], value [n], policy [n][A], noise [A] or NULL: float32 DEVICE pointers of the trainer's device, which must
 * be the calling thread's current one; loss_out: device float[4] = total, evaluation, policy, parameter term, or NULL.
 * noise == NULL and epsilon != 0: A Beta(alpha, 1-alpha) values are drawn (readable afterwards, BB_TRAIN_NOISE).
 * apply = 0 computes loss and gradients only.  lr: the learning rate.  Asynchronous on stream (a hipStream_t; 0 = the default).
 * BB_ERR_ARG: n <= 0, n > max_batch, a required pointer NULL, any pointer not 4-byte aligned. */
int bb_trainer_step(bb_trainer *t, int n, const float *boards, const float *value, const float *policy,
                    const float *noise, double lr, int apply, float *loss_out, void *stream);
/* A whole epoch of steps straight from example records: n_batches times the three launches of bb_trainer_step (apply = 1),
 * enqueued in order as plain launches on `stream` -- no allocation, no host synchronisation, no graph capture, no stream of
 * the trainer's own.  The kernels read the records themselves (csrc/train.hip.h: the records source); no batch tensor exists.
 * Row j of batch i is record order[i * batch + j] under symmetry sym[i * batch + j], decoded exactly as
 * bb_examples_to_batch_sym decodes it: batch i is, bit for bit, the bb_trainer_step the per-batch loop would have made on that
 * call's outputs -- the noise drawn (Philox keyed by the seed and the step count, which advances once per batch, as do Adam's
 * step count and lr_t), the parameters, both slots and the four loss words.  Afterwards BB_TRAIN_GRADS and BB_TRAIN_NOISE read
 * the last batch's.  ALL pointers are device memory of the trainer's device, which must be the calling thread's current one:
 *   records  [n_records][example_bytes] of the trainer's game (the bb_examples_fetch layout), 16-byte aligned
 *   order    [n_batches * batch] int64, or NULL: record i * batch + j
 *   sym      [n_batches * batch] uint8, each < bb_game_symmetries(game), or NULL: the identity
 *   noise    [n_batches][A] float32, or NULL to draw it
 *   loss_out [n_batches][4] float32 (total, evaluation, policy, parameter term of every batch), or NULL
 *   bad_out  [1] int32, incremented by one per malformed row (the caller zeroes it), or NULL
 * A row whose order entry is outside [0, n_records), whose sym entry is not a symmetry of the game or whose record says
 * n_children > S is a row of zeros (planes, label and value) and one count in *bad_out: nothing a record says becomes an
 * address before it has been checked.
 * BB_ERR_ARG, before any device call: a null trainer, n_batches < 0, n_records < 0, batch outside 1..max_batch, a non-finite lr,
 * a misaligned pointer, records NULL or not 16-byte aligned with n_batches > 0, another current device.  n_batches == 0: BB_OK,
 * nothing touched. */
int bb_trainer_epoch(bb_trainer *t, int n_records, const void *records, int n_batches, int batch, const int64_t *order,
                     const uint8_t *sym, const float *noise, double lr, float *loss_out, int32_t *bad_out, void *stream);
/* Score rows with the trainer's current device parameters, forward only (csrc/train_eval.hip.h): no step, no noise, no
 * export.  Nothing of the trainer is written -- not the parameters, the optimiser slots, the gradients, the last step's noise or
 * the step counter that keys the next step's noise --, so a run that evaluates in between its steps trains the same bits.
 * Per row k (a record row exactly as bb_trainer_epoch decodes it: record index[k] under symmetry sym[k]):
 *   rows_out[k] = value (the network's tanh value), se = (value - z)^2, ce = -sum_a pi[a] (logit[a] - max - log sum exp(logit - max))
 *                 with pi the row's policy label; ce is 0 for a row without one (the terminal example: total == 0)
 *   flags_out[k]  bit 0 (BB_ROW_HAS_POLICY) the row has a policy label (some share is not zero; records: total > 0)
 *                 bit 1 (BB_ROW_TOP1)       first maximum of the logits == first maximum of the label (meaningful with bit 0)
 *                 bit 2 (BB_ROW_DECIDED)    z != 0
 *                 bit 3 (BB_ROW_SIGN_OK)    value and z have the same sign (meaningful with bit 2; value == 0 disagrees)
 *                 bit 4 (BB_ROW_COUNTED)        the row is well-formed and takes part in the totals
 * A malformed row (bb_trainer_epoch's definition) writes zeros and flags 0, is counted once in *bad and is in no total.
 * totals_out: counts of the rows with bit 4, bits 0, 0+1, 2, 2+3, and the sums of se over the rows with bit 4 and of ce over
 * those with bit 0, in double: 256 strided partial sums (thread t: rows t, t + 256, ... in order), then a binary tree -- no
 * atomics, the same call gives the same bits.  Layout, 56 bytes, 8-byte aligned: */
typedef struct {
    int64_t rows, policy_rows, top1, decided, sign_ok;
    double se_sum, ce_sum;
} bb_eval_totals;
enum { BB_ROW_HAS_POLICY = 1, BB_ROW_TOP1 = 2, BB_ROW_DECIDED = 4, BB_ROW_SIGN_OK = 8, BB_ROW_COUNTED = 16 };
/* ALL pointers are device memory of the trainer's device, which must be the calling thread's current one; the launches are
 * enqueued on `stream` and not waited for.  Any n >= 0 (max_batch does not bound it: there are no slabs); n == 0 writes zero
 * totals.  records, index, sym: as bb_trainer_epoch's records, order, sym, n entries.  rows_out [n][3] float32 or NULL, flags_out
 * [n] or NULL: without them the per-row figures go to scratch of the trainer's own, which grows to the largest n asked for (a
 * device allocation inside the call, BB_ERR_CAPACITY if it fails).  totals_out is required; bad: [1] int32, incremented, or NULL.
 * BB_ERR_ARG, before any device call: a null trainer or totals_out, a negative count, a misaligned pointer (records 16 bytes,
 * index and totals_out 8, rows_out and bad 4), records NULL with n > 0, another current device. */
int bb_trainer_eval(bb_trainer *t, int n_records, const void *records, int n, const int64_t *index, const uint8_t *sym,
                    float *rows_out, uint8_t *flags_out, bb_eval_totals *totals_out, int32_t *bad, void *stream);
/* The same for rows given as bb_trainer_step's three tensors: boards [n][H][W][C], value [n], policy [n][A], required when n > 0. */
int bb_trainer_eval_tensors(bb_trainer *t, int n, const float *boards, const float *value, const float *policy, float *rows_out,
                            uint8_t *flags_out, bb_eval_totals *totals_out, void *stream);
int bb_trainer_param_count(bb_trainer *t, int64_t *count_out);
/* what = BB_TRAIN_PARAMS | GRADS | SLOT_M | SLOT_V: host_out[count] flat float32, bb_net_weights' fields back to back in their
 * order (the moving statistics included for PARAMS, zero for the others), count = bb_trainer_param_count; SLOT_M is Adam's first
 * moment or Momentum's accumulator, SLOT_V Adam's second moment.  BB_TRAIN_NOISE: the last step's noise, count = A.
 * Synchronises the device.  BB_ERR_ARG for any other `what` or count. */
int bb_trainer_read(bb_trainer *t, int what, float *host_out, int64_t count);
/* bb_load_weights_device with the trainer's own parameter buffer as w_dev: the engine gets the trainer's current weights without
 * a trip through the host, ordered behind the steps queued on `stream` (the stream those steps were given).  Later steps on
 * `stream` wait for the packing.  BB_ERR_ARG, before any device call: a null argument, a trainer and an engine of different games or
 * devices; otherwise bb_load_weights_device's answers. */
int bb_trainer_load_engine(bb_trainer *t, bb_engine *e, void *stream);

/* ---- example records scored with the network an engine holds ------------------------------------ */
/* An extension (the reference has no held-out score), like bb_trainer_eval, which covers the trainer's float32 network of the
 * dense games with 16 filters only.  This call scores records with whatever network the ENGINE evaluates positions with -- the
 * one behind Network.getEvaluation (Network.py:48-54) and the search: the fused 16-filter tower or the launch-per-layer network,
 * in the split-operand or the float32-MFMA form (bb_net_form), for every game -- so the figures are those of the arithmetic
 * that chooses the moves.  csrc/examples_score.hip.h: per chunk of rows a gather of the records' packed states, the engine's own
 * network launch (no noise, no keys, no evaluation cache) and one wave per row for the figures; then bb_trainer_eval's totals
 * launch, unchanged.  Per row k (record index[k]; NULL: record k), as bb_trainer_eval defines them:
 *   rows_out[k] = value (the engine's, unchanged), se and ce by bb_trainer_eval's expressions above, the max and the sum
 *                 over all A logits, pi[a] = (float)((double)visits / (double)total); DragonChess takes pi from the record's
 *                 compact list (visits[j] at action[j], j < n_children) and forms no 4032-wide label row; ce is 0 without a label
 *   flags_out[k]  BB_ROW_*; BB_ROW_HAS_POLICY: total != 0 and some visit count is not zero; BB_ROW_TOP1: first maximum of the
 *                 logits == first maximum of the label in action order (DragonChess: the child with the largest share, ties to
 *                 the smallest action id wherever it stands in the list; duplicate actions are no error, every entry counts)
 * A malformed row -- index[k] outside [0, n_records), n_children > S, a compact action[j] >= A -- is {0, 0, 0} with flags 0, one
 * count in *bad (when non-NULL) and in no total; the network sees the game's initial position in its place, and nothing a record
 * says becomes an address before it has been checked.  All sums run in a fixed order without float atomics: the same call gives
 * the same bits, whatever the chunk size.
 * The scratch memory for chunks of rows_per_chunk rows, in bytes: the gathered states, value[chunk] and logits[chunk][A]; it grows
 * with rows_per_chunk and is a multiple of 16.  Host only: no device call.  BB_ERR_ARG: a null argument, rows_per_chunk < 0. */
int bb_examples_score_workspace(bb_engine *e, int rows_per_chunk, uint64_t *bytes_out);
/* ALL pointers are device memory of the engine's device, which must be the calling thread's current one.  records
 * [n_records][example_bytes] (the bb_examples_fetch layout), index [n] int64 or NULL, rows_out [n][3] float32, flags_out [n],
 * totals_out (56 bytes), bad [1] int32 (incremented; the caller zeroes it) or NULL.  The chunk size is the number of rows the
 * given workspace holds (at most n): any workspace that holds one row gives the same bytes.
 * Ordering: the call waits on the host for the engine's own streams (a score never runs beside a search), makes the engine's
 * stream wait for what `stream` (a hipStream_t; 0 = the default stream) has queued, enqueues everything on the engine's stream and
 * makes `stream` wait for the end.  It does not synchronise `stream`, copies nothing to the host and allocates nothing -- but for
 * the activation buffers of the launch-per-layer network, which grow (and wait) as for any larger batch.  Trees, slots,
 * counters, the evaluation cache and its counters, the random streams and the weights are left alone.
 * n == 0: BB_OK, and the totals launch writes zero totals (there is a GPU: an engine exists).  BB_ERR_ARG, before any device
 * call: a null engine or totals_out, n < 0, n_records < 0, a misaligned pointer (records and workspace 16 bytes, index and
 * totals_out 8, rows_out and bad 4), with n > 0 a null records, rows_out, flags_out or workspace, or a workspace too small for one
 * row.  BB_ERR_WEIGHTS: an engine without loaded weights, or whose evaluator is not the network.  BB_ERR_ARG: another current
 * device. */
int bb_examples_score(bb_engine *e, int n_records, const void *records, int n, const int64_t *index, float *rows_out,
                      uint8_t *flags_out, bb_eval_totals *totals_out, int32_t *bad, void *workspace, uint64_t workspace_bytes,
                      void *stream);

#ifdef __cplusplus
}
#endif
#endif
