/* evg_dqn.h -- the acting turn of the reference's base agent family, agents/DQN: QNetwork(105 -> h1 -> 132) on the raw 105-word observation, the
 * 132-way head's decode (DQNAgent.filter_actions) and the exploring turn (DQNAgent.epsilon_greedy): the entry points libevg_dqn.so adds to those of
 * libevg.so. */
#ifndef EVG_DQN_H
#define EVG_DQN_H
#include "evg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Three functions under ABI 7.  They are NOT part of libevg.so, whose entry points are exactly those of evg.h: `make dqn` builds libevg_dqn.so from the
 * same sources with -DEVG_DQN, which exports evg.h's entry points plus these three.  A handle made by either library is valid in the other (same
 * sources, one HIP runtime); an error's text is read with the evg_last_error of the library whose call failed.  Every call is asynchronous on
 * `stream`, allocates nothing, synchronises nothing and can be captured. */

#define EVG_DQN_IN 105              /* the observation (EVG_OBS_LEN)                                                                    */
#define EVG_DQN_OUT 132             /* the head: Q[group * 11 + node], 12 groups x 11 nodes                                             */
#define EVG_DQN_MAX_HIDDEN 528      /* fc1_unit of agents/DQN/QNetwork.py; any h1 in 1..528 is evaluated                                */
#define EVG_DQN_CHUNK 48            /* hidden units per staged chunk of the weights (see NETWORK below)                                 */
#define EVG_DQN_TINY_ROWS 4096      /* up to here a workgroup pass is ONE 16-row group, shared by the workgroup's four wavefronts       */
#define EVG_DQN_SMALL_ROWS 16384    /* up to here a workgroup pass is 64 rows (one 16-row group per wavefront), beyond it 256 rows (four) */
#define EVG_DQN_MAX_BLOCKS 256      /* the grid's cap: workgroups stride over the row blocks beyond it                                  */

/* evg_dqn_qnet's input forms */
#define EVG_DQN_ROWS 0              /* x is float32 [rows][105]                                                                         */
#define EVG_DQN_OBS_SEAT 1          /* x is a one-seat observation buffer [rows][105] in the handle's obs_dtype                         */
#define EVG_DQN_OBS 2               /* x is a two-seat observation buffer [rows][2][105] in the handle's obs_dtype; `seat` picks [:, seat] */

/* The network's parameters: device pointers the caller owns, nn.Linear layout, fp32, 16-byte aligned, read in place at every call. */
typedef struct evg_dqn_net {
    uint32_t struct_size;          /* sizeof(evg_dqn_net)                                          */
    int32_t h1;                    /* hidden size, 1..EVG_DQN_MAX_HIDDEN                           */
    int32_t final_relu;            /* 1: QNetwork.forward's ReLU on the output (the reference), 0  */
    int32_t reserved;              /* 0                                                            */
    const float* w1;               /* [h1][105]                                                    */
    const float* b1;               /* [h1]                                                         */
    const float* w2;               /* [132][h1]                                                    */
    const float* b2;               /* [132]                                                        */
} evg_dqn_net;

/* NETWORK.  q_out float32 [rows][132] = relu?(W2 . relu(W1 . x + b1) + b2), rows in 1..EVG_QNET_MAX_ROWS, one launch.
 *
 * Numeric contract (tests/dqn_model.py restates it): the library's fp32 chain.  Every pre-activation is acc = b[j], then acc = fmaf(W[j][k], x[k], acc)
 * for k ascending over ALL of k -- 0..104 in layer 1, 0..h1-1 in layer 2 --, then torch's ReLU, acc < 0 ? 0 : acc (a NaN stays a NaN), on the hidden
 * layer and, with final_relu, on the output.  The sign of a zero is not part of the contract.  Two calls give bit-equal Q; there is no floating-point
 * atomic.  An observation element of the forms EVG_DQN_OBS_SEAT / EVG_DQN_OBS is converted on load as x.float() converts it (float64: round to nearest
 * even; int16: exact).
 *
 * The 501 KB of fp32 weights fit neither LDS nor registers, so the hidden layer is streamed in chunks of EVG_DQN_CHUNK units: a workgroup stages W1's
 * rows and W2's columns of the chunk in LDS, runs layer 1 of the chunk and continues layer 2's 132 accumulators with the chunk's k, chunks ascending:
 * the chain above, unchanged.  Padded positions -- input columns 105..107, hidden units >= h1, outputs >= 132 -- enter the matrix core as exact zeros
 * by selection, never by a product with zero: a non-finite x or weight does not leak through padding.  Nothing is read past the last row's 105th
 * element and nothing outside [rows][132] is written.
 *
 * Grid: a workgroup pass takes 16 rows up to EVG_DQN_TINY_ROWS rows (its wavefronts share the group: three run layer 1's column tiles, all four deal
 * layer 2's output tiles), 64 rows up to EVG_DQN_SMALL_ROWS rows and 256 rows beyond; min(passes, EVG_DQN_MAX_BLOCKS) workgroups stride over them.
 * The three forms compute the same chain: a row's Q does not depend on how many rows the call has.
 *
 * Refused with EVG_ERR_INVALID (nothing launched): a NULL handle, descriptor, x or q_out; struct_size != sizeof(evg_dqn_net); h1 outside
 * 1..EVG_DQN_MAX_HIDDEN; final_relu not 0/1; an unknown input form; seat outside 0..1 (EVG_DQN_OBS); rows outside 1..EVG_QNET_MAX_ROWS; a NULL or
 * not 16-byte aligned parameter pointer; x or q_out not 16-byte aligned. */
EVG_API int evg_dqn_qnet(evg_handle* h, const evg_dqn_net* net, int input, int seat, int64_t rows, const void* x, float* q_out, void* stream);

/* DECODE.  DQNAgent.filter_actions (agents/DQN/DQNAgent.py:161-197) for every env of the handle: q float32 [N][132] -> actions_out int32 [N][7][2] of
 * {unit, node}, every quirk kept.  Three arrays of seven start at zero: best_q, unit, node.  For node 0..10, for group 0..11, for slot i 0..6: if
 * q[group * 11 + node] > best_q[i] then -- if group is among the seven unit values (an unfilled slot counts as unit 0) and unit[i] != group, go on to
 * the next slot -- otherwise store q, group and node in slot i and leave the slot loop.  Row i is {unit[i], node[i]} with node in 0..10 as the
 * reference returns it (no + 1, no repair of node 0).  A NaN or a q <= 0 is never taken, so an all-zero row decodes to seven {0, 0}.  Comparisons are
 * on the fp32 values.  One env per lane, the seven slots in registers.
 * Refused with EVG_ERR_INVALID: a NULL argument, q or actions_out not 16-byte aligned. */
EVG_API int evg_dqn_actions(evg_handle* h, const float* q, int32_t* actions_out, void* stream);

/* EXPLORING TURN.  DQNAgent.epsilon_greedy (:131-159) for every env: the coin, then the random branch or filter_actions.  The draws are those of RNG
 * domain 4 exactly as evg_minimized_get_action uses them -- key (env id, episode, turn, seat), the turn and episode the handle's, blocks 0 and 1, the
 * coin (half 7 of block 0 << 16 | half 7 of block 1), the 7 distinct units from halves 0..6 of block 0 and the 7 distinct nodes from halves 0..6 of
 * block 1 by partial Fisher-Yates (a seat runs one agent family per turn) -- with the reference's two differences: the node is the drawn element
 * itself, 0..10 (np.random.choice(11, 7, replace=False), no + 1), and the test is `sample > eps` means greedy, so an env explores iff
 * coin / 2^32 <= eps, compared in float64.  epsilon: one value in [0, 1] for every env, unless epsilon_env (device float32 [N]) gives one per env.
 * The decay schedule of eps_threshold and the global steps_done stay the caller's.  explored_out: NULL or device uint8 [N], 1 where the random branch
 * ran, written for every env.
 * Refused with EVG_ERR_INVALID: a NULL handle, q or actions_out; seat outside 0..1; an epsilon outside [0, 1]; q or actions_out not 16-byte aligned; a
 * handle in the stock-entropy mode (the draws are keyed). */
EVG_API int evg_dqn_get_action(evg_handle* h, const float* q, float epsilon, const float* epsilon_env, int seat, int32_t* actions_out,
                               uint8_t* explored_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
