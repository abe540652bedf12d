// pw_kernels_critic.hpp -- part of libpworld.so (translation unit csrc/pworld_critic.hip includes it).
// The learner's critic (rls/model/ac_network_multi_gumbel.py CriticNetwork) as ONE launch: dense1 + ReLU on [obs | action], a
// one-layer LSTM (hidden 64) over the agent axis, dot-product attention of every step's output against the final hidden state,
// softmax over the agents, weighted sum, ReLU, dense2 -> q [b]; optionally the TD target y = r + gamma q (1 - d) from the same q.
//
// Design (the one-launch actor's, pw_kernels_actor16.hpp / pw_kernels_policy3.hpp, restated for a unidirectional 64-unit LSTM):
//   * a workgroup of 512 threads owns R batch rows (R = 16; 8 when N > 32, see "LDS") = the 16 columns of v_mfma_f32_16x16x4_f32;
//   * wave w owns hidden units 8 w .. 8 w + 7 as two 16-row tiles, tile row = 4 (unit within tile) + gate: after the matrix
//     instructions a lane's four accumulator registers ARE the gates i, f, g, o of one unit for one batch row, so the cell update
//     (lstm_cell of pw_lstm_math.hpp: fast_sigmoid / fast_tanh) needs no exchange.  W_ih and W_hh of the wave's 32 gate rows
//     stay in registers for the whole launch (64 per lane; + the wave's W1 tile, up to 30), read straight from the nn.Module layout [256][64];
//   * dense1 runs just in time as 16 x 16 tiles (hidden quarter x batch rows, K = D + A): waves 0-3 produce timestep t + 2 and
//     waves 4-7 timestep t + 3 during every even step t, into a ring of four x1 buffers in B-fragment order; the observation row
//     is requested at the top of the step and consumed after the step's own matrix work.  An action given as indices is fed as
//     the one-hot B operand built in registers (1.0f where the action column = index): the matrix instruction then adds exactly the weight
//     column -- the same instruction, operands and order as an exact one-hot act_vec, hence the same bits -- and no one-hot tensor
//     exists in memory.  The obs part and the action part of K are separate k steps (each zero-padded to a whole number of them);
//   * the input projection of step t + 1 is issued before the barrier of step t (it does not depend on the recurrence);
//   * every step's output h_t stays in LDS in the B-fragment order of the recurrence (the buffer of step t - 1 IS the h exchange),
//     so the attention pass reads it back with conflict-free 16-byte reads: scores by wave (t = wave, wave + 8, ..), softmax
//     statistics redundantly per wave in registers, the context of a lane's own two units, dense2 as a two-stage reduction.
// LDS: N R 256 bytes of step outputs + 4 x1 buffers (R KB) + scores: R = 16 serves N <= 32 (146.5 KiB at N = 32), longer agent axes
// run 8 rows per workgroup (columns 8 .. 15 of the tiles idle; 140.5 KiB at N = 64).  Nothing between the input rows and q touches HBM.
//
// The per-step critic (rls/model/ac_network_multi_gumbel_BIC.py CriticNetwork, the BiCNet baseline) is the same front end and
// recurrence with a head on every step's output instead of the attention: q[r][t] = <w2, h_t[r]> + b2 (no ReLU), and the TD
// target per agent.  It is the third template parameter of the one kernel (pw_critic_forward_kernel<KO, KA, STEPS>), not a copy:
//   * only h_{t-1} and h_t are live, so the step outputs are a TWO-slot ring (slot t & 1) and R = 16 rows per workgroup serve
//     every N <= 64 (critic_steps_lds: 8 KB of step outputs + 16 KB of x1 buffers + the q staging, 28 KB at N = 64);
//   * the head runs IN the loop: during step t + 1 wave t % 8 forms q_t from the B fragments of h_t every wave has just read for
//     the recurrence (its own 16 units in ascending order, then the two lane_xor exchanges: a fixed order that does not depend on
//     N), behind the step's matrix instructions; the last step's head follows the loop.  q_t is staged in LDS as [row][N] so that q
//     (and y) leave at the end in whole [row][0 .. N) runs -- the workgroup's rows are one contiguous run of rows_here * N floats
//     -- instead of 16 scattered 4-byte stores per step.  (Chosen from the store pattern, not from a measurement: per-step
//     stores were not timed.)
//   INVARIANT of the ring: the slot of h_t (t & 1) is rewritten by step t + 2, i.e. only after the barrier of step t + 1; every
//   read of h_t -- the recurrence of step t + 1 and the head of q_t, both in step t + 1 -- comes before that barrier.
//
// The model-learning critic (rls/model/ac_network_model_multi_gumbel.py CriticNetwork, the paper's own method) is the attention
// critic without the ReLU on the context and with a second head: q = <w2, ctx> + b2 and r_pred = <w3, ctx> + b3.  It is the
// third form of the one kernel body (MODEL; pw_critic_forward_kernel<KO, KA>(CriticModelArgs)): front end, recurrence, scores, softmax and context
// are the attention form's lines, and both heads are summed in q's order (a lane's two units, lane_xor16, lane_xor32, the eight
// wave partials ascending, the bias), so w3 = w2, b3 = b2 gives r_pred the bits of q.  r_pred == NULL (the target critic) skips the
// second head.  Same LDS layout (critic_lds) and the same R rule.
#pragma once

#include "pw_common.hpp"
#include "pw_lstm_math.hpp"

namespace {

struct CriticArgs {
    const float *obs;        // [b][N][D]
    const int32_t *act_idx;  // [b][N][heads] or NULL
    const float *act_vec;    // [b][N][A] or NULL
    const float *w1, *b1;    // dense1.module: [64][D + A], [64]
    const float *w_ih, *w_hh, *b_ih, *b_hh;  // lstm: [256][64] x 2, [256] x 2 (gate order i, f, g, o)
    const float *w2, *b2;    // dense2: [1][64], [1]
    const float *rew, *done; // [b] each or NULL
    float *q, *y;            // [b]; y or NULL
    long b;
    int N, D, A, n0, n1, R;
    float gamma;
};

// the model-learning critic: a second head on the same context
struct CriticModelArgs : CriticArgs {
    const float *w3, *b3;    // dense3: [1][64], [1]; unread when r_pred is NULL
    float *r_pred;           // [b] or NULL
};
__device__ __forceinline__ const CriticModelArgs *critic_model_args(const CriticArgs &) { return nullptr; }
__device__ __forceinline__ const CriticModelArgs *critic_model_args(const CriticModelArgs &C) { return &C; }

struct CriticLds { float4 *s_out, *s_x; float *s_sc, *s_red; uint32_t bytes; };
__host__ __device__ inline CriticLds critic_lds(int N, int R, unsigned char *raw = nullptr)
{
    LdsCursor c{reinterpret_cast<float *>(raw)}; CriticLds o;
    // [N][4 j][FR = 4 R]: element e of slot (kq, n) = h_t[unit 16 j + 4 e + kq][row n]; [4 buffers][4 j][FR]: the same order for x1 = relu(dense1)
    o.s_out = c.take<float4>(N * 4 * 4 * R); o.s_x = c.take<float4>(4 * 4 * 4 * R);
    o.s_sc = c.take<float>(N * 16); o.s_red = c.take<float>(8 * 16);   // [N][16] attention scores, [8 waves][16] dense2 partial sums
    o.bytes = 4 * c.at; return o;
}

// The per-step critic's layout: R = 16 for every N.  [2 slots][4 j][FR]: h_t in slot t & 1, the order of critic_lds; the four x1 buffers;
// [R][N] q staging (row-major: what leaves for q / y).
struct CriticStepsLds { float4 *s_out, *s_x; float *s_q; uint32_t bytes; };
__host__ __device__ inline CriticStepsLds critic_steps_lds(int N, int R, unsigned char *raw = nullptr)
{
    LdsCursor c{reinterpret_cast<float *>(raw)}; CriticStepsLds o;
    o.s_out = c.take<float4>(2 * 4 * 4 * R); o.s_x = c.take<float4>(4 * 4 * 4 * R);
    o.s_q = c.take<float>(R * N);
    o.bytes = 4 * c.at; return o;
}
template <bool STEPS>
__device__ __forceinline__ auto critic_layout(const int N, const int R, unsigned char *raw)
{
    if constexpr (STEPS) return critic_steps_lds(N, R, raw);
    else return critic_lds(N, R, raw);
}

// KO / KA: k steps of dense1 (four k each) the instantiation holds for the observation and the action part: ceil(D / 4) <= KO,
// ceil(A / 4) <= KA.  (Both compile-time, so that every operand address is one per-lane pointer + an immediate: with the split at
// a run-time k step the compiler keeps a hoisted address pair per operand across the timestep loop, and spills.)
// STEPS: the per-step critic, pw_critic_forward_steps (rew / done / q / y are [b][N]); else the attention critic, pw_critic_forward.  One
// kernel template for both: the discarded branches leave no trace, so the <KO, KA, false> instantiations are, instruction for
// instruction, the attention kernel as it was before the per-step form existed.
// MODEL: the model-learning critic, pw_critic_forward_model.  A compile-time constant of the one body like STEPS, but not a fourth
// parameter of this template: a parameter more renames the sixteen kernels there were (tools/code_object.py --compare pairs a
// build's kernels with its parent's by name), and the body as a __forceinline__ function called from two kernels compiles to other
// instructions than the body in the kernel (other register numbers, 8 to 11 instructions fewer: tried with the argument block by
// reference and by value).  So the body is text, pw_kernels_critic_body.inc, included by the template the per-step form made and
// by an overload of it that carries the form in its signature (two parameters, CriticModelArgs).
template <int KO, int KA, bool STEPS>
__global__ void __launch_bounds__(512) pw_critic_forward_kernel(const CriticArgs C)
{
    constexpr bool MODEL = false;
#include "pw_kernels_critic_body.inc"
}

template <int> constexpr bool critic_no = false;
template <int KO, int KA>
__global__ void __launch_bounds__(512) pw_critic_forward_kernel(const CriticModelArgs C)
{
    // value-dependent, so that `if constexpr (STEPS)` leaves its branch uninstantiated (it names members critic_lds's layout lacks)
    constexpr bool STEPS = critic_no<KO>, MODEL = true;
#include "pw_kernels_critic_body.inc"
}


}  // namespace
