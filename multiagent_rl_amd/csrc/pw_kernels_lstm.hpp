// pw_kernels_lstm.hpp -- part of libpworld.so (translation unit csrc/pworld_lstm.hip includes it).
// The recurrent part of a one-layer LSTM WITH gradient, for the learner's three passes per update (critic(s0, a0), actor(s0),
// critic(s0, actor(s0))): pw_lstm_train_forward_kernel walks the steps and keeps what the backward needs (the four gates after
// their activations -- see saved_sigmoid -- and c of every step), pw_lstm_train_backward_kernel walks them in reverse and returns the gradient at the
// pre-activations.  The input projection G = x W_ih^T + b_ih + b_hh and its gradient are GEMMs and stay with the caller (rocBLAS
// through autograd; multiagent_rl_amd/lstm.py); the W_hh gradient is the caller's GEMM too, or pw_lstm_train_wgrad_kernel
// (pw_kernels_lstm_wgrad.hpp, a unit of its own).  One launch each instead of MIOpen's ~45 per direction and pass.
//
// Two shapes, the two the reference's networks have: <H = 64, DIRS = 1> (both critics) and <H = 32, DIRS = 2> (the actor; direction 1
// walks t = N - 1 .. 0).  Mapping, the same for both kernels and both shapes:
//   * lane = (sequence, direction, hidden unit j); the H lanes of a (sequence, direction) sit in ONE wave, so every hand-off
//     between them is wave-private LDS behind wave_lds_sync(), and no workgroup barrier exists after the weights are staged;
//   * W_hh is staged once per workgroup in LDS as float4 runs that the H lanes of a group read at consecutive 16-byte slots
//     (conflict-free), and is read from there every step.  At H = 64 a lane's 4 x 64 weights do not fit its registers beside the
//     working set without spilling; from LDS both shapes run the same code with ~40 registers.  At the learner's shapes
//     (b = 1024, N <= 12: one to two waves per SIMD, a few thousand cycles) the LDS reads of a launch are microseconds and the
//     launch count is what the time is made of;
//     forward:  s_w[dir][k / 4][gate][unit] = W[gate H + unit][k .. k + 3]   (a row of W_hh against h, k ascending)
//     backward: s_w[dir][r / 4][unit]       = W[r .. r + 3][unit]            (a COLUMN of W_hh against dG, r ascending)
//   * the vector every lane of a group needs (h [H] forward, dG_t [4 H] backward) goes through s_x, one slot per group, read back as
//     broadcast float4.
// Summation order is fixed (no atomics): the forward's four gate sums run over k ascending, each a chain of fused multiply-adds that
// starts from the pre-activation; the backward's dh[j] is four partial sums over r = 4 q + e (e = 0 .. 3, q ascending) added as
// (p0 + p1) + (p2 + p3).  Two runs give the same bits.  Weights are read with 4-byte loads (views into nn.LSTM's flat buffer).
// A workgroup's slots past the last sequence compute on sequence 0 and store nothing.
#pragma once

#include "pw_common.hpp"
#include "pw_lstm_math.hpp"

namespace {

constexpr int kLstmThreads = 256;

// s_w: one W_hh per direction, DIRS * H * H float4 (both orders above have this size); s_x: [groups = 256 / H][H or 4 H].
struct LstmTrainLds { float4 *s_w; float *s_x; uint32_t bytes; };
__host__ __device__ inline LstmTrainLds lstm_train_lds(int H, int dirs, bool backward, unsigned char *raw = nullptr)
{
    LdsCursor c{reinterpret_cast<float *>(raw)}; LstmTrainLds o;
    o.s_w = c.take<float4>(dirs * H * H);
    o.s_x = c.take<float>((kLstmThreads / H) * (backward ? 4 * H : H));
    o.bytes = 4 * c.at; return o;
}

// The gates as the backward needs them.  It multiplies by s (1 - s) and 1 - g^2, differences of numbers near 1 once a gate saturates, so what
// counts there is the RELATIVE accuracy of 1 - s, and fast_sigmoid / fast_tanh (pw_lstm_math.hpp: 1 / (1 + e), 2 / (1 + e) - 1) round 1 + e and
// its reciprocal at the size of 1: measured, a backward fed those values was 4.3 x stock float32's error at saturated gates over 64 steps, fed
// exact gates 1.04 x (profiles/lstm_train_saturated.txt).  So the SAVED copy is formed from the small side: q = e / (1 + e) with
// e = exp(-|x|) <= 1 carries a few ulp of relative error however small it is, and the gate is q or 1 - q (tanh: e = exp(-2 |x|), 1 - 2 q with
// the sign of x); the difference from the value the cell used for c and h is the last bits (<= ~2.5e-7).  c and h stay
// lstm_cell_train's (below), bit for bit with and without saving.  Finite for every finite x: e in [0, 1], 1 + e in [1, 2].
__device__ __forceinline__ float saved_sigmoid(const float x)
{
    const float e = __builtin_amdgcn_exp2f(fabsf(x) * -1.4426950408889634f);
    const float q = e / (1.0f + e);
    return x >= 0.0f ? 1.0f - q : q;
}
__device__ __forceinline__ float saved_tanh(const float x)
{
    const float e = __builtin_amdgcn_exp2f(fabsf(x) * -2.8853900817779268f);
    return copysignf(1.0f - 2.0f * (e / (1.0f + e)), x);
}

// The cell of the passes with gradient.  fast_tanh forms 2 / (1 + e) - 1, a difference of numbers near 1: its ABSOLUTE error is one rounding
// of 1 (~1e-7) however small the value is, and with the learner's pre-activations tanh(g) and tanh(c) are a few tenths and less -- the LSTM
// output then carried 3.4 x MIOpen's rms error, part of it of one sign, which the row sums of the layers behind it keep (the critic's
// dense2.weight gradient was 4.97 x stock float32's against float64 in a whole update, tests/test_gpu_update_parity.py).  Here both are
// tanhf, accurate relative to the value; the sigmoids are lstm_cell's operations (a gate near 0.5 has that rounding anyway).  The no-gradient
// kernels keep lstm_cell.
__device__ __forceinline__ float train_tanh(const float x) { return tanhf(x); }
__device__ __forceinline__ void lstm_cell_train(const float gi, const float gf, const float gg, const float go, float &c, float &h)
{
    const float si = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(gi * -1.4426950408889634f));
    const float sf = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(gf * -1.4426950408889634f));
    const float so = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(go * -1.4426950408889634f));
    c = sf * c + si * train_tanh(gg);
    h = so * train_tanh(c);
}

// G [b][N][DIRS][4 H], Y [b][N][DIRS H], saved [b][N][DIRS][5][H] (i, f, g, o after activation, c) or NULL
template <int H, int DIRS>
__global__ void __launch_bounds__(kLstmThreads) pw_lstm_train_forward_kernel(const float *__restrict__ G, const float *__restrict__ w_fw,
                                                                             const float *__restrict__ w_bw, const long b, const int N,
                                                                             float *__restrict__ Y, float *__restrict__ saved)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lstm_smem[];
    const LstmTrainLds S = lstm_train_lds(H, DIRS, false, lstm_smem);
    float *sw = reinterpret_cast<float *>(S.s_w);
    for (int e = threadIdx.x; e < DIRS * 4 * H * H; e += kLstmThreads) {
        const int d = e / (4 * H * H), r = e % (4 * H * H), row = r / H, k = r % H, gate = row / H, unit = row % H;
        sw[((((d * (H / 4) + (k >> 2)) * 4 + gate) * H + unit) << 2) + (k & 3)] = (d ? w_bw : w_fw)[r];
    }
    __syncthreads();
    const int j = threadIdx.x % H, grp = threadIdx.x / H;
    const long gid = (long)blockIdx.x * (kLstmThreads / H) + grp;   // group = sequence * DIRS + direction
    const bool valid = gid < b * DIRS;
    const size_t seq = valid ? (size_t)(gid / DIRS) : 0;
    const int dir = valid ? (int)(gid % DIRS) : 0;
    const float4 *w = S.s_w + dir * H * H + j;
    float *hs = S.s_x + grp * H;
    float h = 0.0f, c = 0.0f;
    const float *g0 = G + ((seq * N + (dir ? N - 1 : 0)) * DIRS + dir) * 4 * H;
    float ni = g0[j], nf = g0[H + j], ng = g0[2 * H + j], no = g0[3 * H + j];
    for (int s = 0; s < N; ++s) {
        const int t = dir ? N - 1 - s : s;
        float ai = ni, af = nf, ag = ng, ao = no;
        if (s + 1 < N) {   // the next step's pre-activations travel under this step's sums
            const float *g = G + ((seq * N + (dir ? t - 1 : t + 1)) * DIRS + dir) * 4 * H;
            ni = g[j]; nf = g[H + j]; ng = g[2 * H + j]; no = g[3 * H + j];
        }
        if (s > 0) {       // h = 0 before the first step: the sums would add nothing
            hs[j] = h;
            wave_lds_sync();
#pragma unroll 4
            for (int q = 0; q < H / 4; ++q) {
                const float4 hv = reinterpret_cast<const float4 *>(hs)[q];
                const float4 wi = w[(q * 4 + 0) * H], wf = w[(q * 4 + 1) * H], wg = w[(q * 4 + 2) * H], wo = w[(q * 4 + 3) * H];
                ai = fmaf(wi.x, hv.x, ai); af = fmaf(wf.x, hv.x, af); ag = fmaf(wg.x, hv.x, ag); ao = fmaf(wo.x, hv.x, ao);
                ai = fmaf(wi.y, hv.y, ai); af = fmaf(wf.y, hv.y, af); ag = fmaf(wg.y, hv.y, ag); ao = fmaf(wo.y, hv.y, ao);
                ai = fmaf(wi.z, hv.z, ai); af = fmaf(wf.z, hv.z, af); ag = fmaf(wg.z, hv.z, ag); ao = fmaf(wo.z, hv.z, ao);
                ai = fmaf(wi.w, hv.w, ai); af = fmaf(wf.w, hv.w, af); ag = fmaf(wg.w, hv.w, ag); ao = fmaf(wo.w, hv.w, ao);
            }
            wave_lds_sync();   // every read of h done before the next step overwrites it
        }
        lstm_cell_train(ai, af, ag, ao, c, h);
        if (valid) {
            Y[(seq * N + t) * (DIRS * H) + dir * H + j] = h;
            if (saved) {
                float *sv = saved + ((seq * N + t) * DIRS + dir) * 5 * H;
                sv[j] = saved_sigmoid(ai); sv[H + j] = saved_sigmoid(af); sv[2 * H + j] = saved_tanh(ag); sv[3 * H + j] = saved_sigmoid(ao);
                sv[4 * H + j] = c;
            }
        }
    }
}

// What one step of the backward reads: the saved gates and c, and dY of the unit.
struct LstmSavedStep { float i, f, g, o, c, dy; };
template <int H, int DIRS>
__device__ __forceinline__ LstmSavedStep lstm_saved_step(const float *__restrict__ saved, const float *__restrict__ dY, const size_t seq,
                                                          const int N, const int t, const int dir, const int j)
{
    const float *sv = saved + ((seq * N + t) * DIRS + dir) * 5 * H;
    return {sv[j], sv[H + j], sv[2 * H + j], sv[3 * H + j], sv[4 * H + j], dY[(seq * N + t) * (DIRS * H) + dir * H + j]};
}

// dY [b][N][DIRS H], saved as the forward wrote it, dG [b][N][DIRS][4 H]
template <int H, int DIRS>
__global__ void __launch_bounds__(kLstmThreads) pw_lstm_train_backward_kernel(const float *__restrict__ dY, const float *__restrict__ saved,
                                                                              const float *__restrict__ w_fw, const float *__restrict__ w_bw,
                                                                              const long b, const int N, float *__restrict__ dG)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lstm_smem[];
    const LstmTrainLds S = lstm_train_lds(H, DIRS, true, lstm_smem);
    float *sw = reinterpret_cast<float *>(S.s_w);
    for (int e = threadIdx.x; e < DIRS * 4 * H * H; e += kLstmThreads) {
        const int d = e / (4 * H * H), r = e % (4 * H * H), row = r / H, k = r % H;
        sw[(((d * H + (row >> 2)) * H + k) << 2) + (row & 3)] = (d ? w_bw : w_fw)[r];
    }
    __syncthreads();
    const int j = threadIdx.x % H, grp = threadIdx.x / H;
    const long gid = (long)blockIdx.x * (kLstmThreads / H) + grp;
    const bool valid = gid < b * DIRS;
    const size_t seq = valid ? (size_t)(gid / DIRS) : 0;
    const int dir = valid ? (int)(gid % DIRS) : 0;
    const float4 *w = S.s_w + dir * H * H + j;
    float *ds = S.s_x + grp * 4 * H;
    float dh = 0.0f, dc = 0.0f;
    LstmSavedStep cur = lstm_saved_step<H, DIRS>(saved, dY, seq, N, dir ? 0 : N - 1, dir, j);
    for (int s = N - 1; s >= 0; --s) {   // s: the step's place in the forward order
        const int t = dir ? N - 1 - s : s;
        LstmSavedStep prev = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // c_prev = 0 at the forward's first step
        if (s > 0) prev = lstm_saved_step<H, DIRS>(saved, dY, seq, N, dir ? t + 1 : t - 1, dir, j);
        const float tc = train_tanh(cur.c);
        const float dht = cur.dy + dh;
        const float d_o = dht * tc * (cur.o * (1.0f - cur.o));
        const float dct = dc + dht * cur.o * (1.0f - tc * tc);
        const float d_i = dct * cur.g * (cur.i * (1.0f - cur.i));
        const float d_f = dct * prev.c * (cur.f * (1.0f - cur.f));
        const float d_g = dct * cur.i * (1.0f - cur.g * cur.g);
        if (valid) {
            float *o = dG + ((seq * N + t) * DIRS + dir) * 4 * H;
            o[j] = d_i; o[H + j] = d_f; o[2 * H + j] = d_g; o[3 * H + j] = d_o;
        }
        dc = dct * cur.f;
        if (s > 0) {   // dh of the step before: dG_t . W_hh, this unit's column
            ds[j] = d_i; ds[H + j] = d_f; ds[2 * H + j] = d_g; ds[3 * H + j] = d_o;
            wave_lds_sync();
            float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f, p3 = 0.0f;
#pragma unroll 8
            for (int q = 0; q < H; ++q) {
                const float4 dv = reinterpret_cast<const float4 *>(ds)[q];
                const float4 wv = w[q * H];
                p0 = fmaf(dv.x, wv.x, p0); p1 = fmaf(dv.y, wv.y, p1); p2 = fmaf(dv.z, wv.z, p2); p3 = fmaf(dv.w, wv.w, p3);
            }
            wave_lds_sync();   // every read of dG_t done before the next step overwrites it
            dh = (p0 + p1) + (p2 + p3);
        }
        cur = prev;
    }
}

}  // namespace
