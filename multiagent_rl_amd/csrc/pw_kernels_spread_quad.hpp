// pw_kernels_spread_quad.hpp -- part of libpworld.so (translation unit csrc/pworld.hip includes it).
// simple_spread N = L = 6 on small grids (the latency-bound regime of BASELINE configs[1]): four cooperating waves.
#pragma once

#include "pw_kernels_spread.hpp"

namespace {

// ------------------------------------------------------------------------------------------
// At B = 4096 a step of pw_spread_duo_kernel is ONE wave's dependent chain (wave P: ~1930 cycles, a third of them
// issue slots; profiles/r2_c2_b4096_duo_summary.json): a lane owns an agent, loops over its near partners one after
// the other (~600 cycles of dependent float32 work per partner), then a second pass over all partners finds the next
// step's near set; the output wave O needs ~1500 cycles for its own chain of LDS exchanges.  The chip has four times
// more lanes than this batch has agents, so this kernel spends lanes to shorten both chains:
//   waves P0, P1  physics of 4 envs each, PAIR-parallel: lane = one of the env's 15 unordered agent pairs (60 lanes).
//                 Every pair is tested and, if near, evaluated ONCE, all pairs at the same time -- no per-lane partner
//                 loop, no separate near-set pass; the pair's force goes to the first agent, its exact negation (IEEE:
//                 delta, quotients and products only change sign) to the second, through a [agent][partner] table in
//                 LDS (wave shuffles were measured: slower); the env's 6 agent lanes then add their row in ascending partner order (the upstream
//                 accumulation order, so the bits do not change; far pairs contribute +-0, which cannot change an
//                 accumulator that is never -0), integrate and publish {pos, vel} into the ring.
//   wave OA       8 envs, one step behind (as the duo kernel's O): landmark minima, rewards, shared reward.
//   wave OB       8 envs, one step behind: observation rows, stored as one contiguous block per step
//                 (stream_write_obs_block), and the pre-reset rows at episode ends; done / terminal stores; the collision
//                 tests (counts handed to OA through LDS one step later, masks stored) -- the two output waves issue
//                 about the same number of vector instructions per step (profiles/r7_quad_loop_census.txt); and the
//                 physics waves' action force: OB fetches the action indices (LDS-direct loads, four iterations ahead),
//                 looks the force up in a six-entry table and leaves it in a two-slot LDS ring TWO steps ahead of the
//                 physics waves, which read it with one LDS load at the top of a step (steps 0 and 1 of a launch they
//                 fetch and decode themselves, before the loop).  No meeting of its own: the entry of step t + 2 is
//                 written between barriers t and t + 1 and read behind barrier t + 1; its slot's previous entry was
//                 consumed before barrier t (profiles/r8_quad_actions.txt, r8_quad_loop_census.txt).
// One s_barrier per step.  The ring slot sequence is WORKGROUP-uniform: in a step in which ANY of the 8 envs resets,
// every env publishes a pre-reset and a post-reset slot (identical for the envs that do not reset), so no wave needs
// another env's slot index; each wave follows all 8 episode clocks itself.  Envs out of step with each other can make
// that happen in consecutive steps, so the ring has 4 slots: the two the output waves are reading (one step behind)
// and the two the physics waves may be writing.
// Per-step overheads are kept off the physics waves' instruction stream: the episode clocks are offsets behind ONE scalar
// compare per step (the vector work runs in reset steps only), the action force arrives ready-made from wave OB (the
// physics waves' step loop holds no vector memory operation, no vmcnt wait and no M0 statement), the pair operands of the
// next step are read back before the barrier.  Measured state (profiles/r2_action_prefetch.txt, r2_c2_b4096_quad_summary.json):
// 0.62 us per step at B = 4096, the three kinds of waves within 10 % of each other, 0.53 us for a lone workgroup.
// Arithmetic and results are identical to the other simple_spread kernels (same bit-exact tests, `quad` path).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void quad_pair_of(const int q, int &i, int &j)
{
    // unordered pairs of 6 agents in lexicographic order: (0,1) (0,2) ... (0,5) (1,2) ... (4,5)
    i = q < 5 ? 0 : q < 9 ? 1 : q < 12 ? 2 : q < 14 ? 3 : 4;
    j = q - (i == 0 ? 0 : i == 1 ? 5 : i == 2 ? 9 : i == 3 ? 12 : 14) + i + 1;
}

// Wave OB's action fetch (pw_common.hpp act_fetch_issue, which the duo / tag kernels keep in their physics waves): the same
// LDS-direct load in its scalar-base form -- `row` is the workgroup-uniform pointer to the step's action plane, a running pointer
// of the caller's, `lane_off` the lane's constant byte offset in it -- so a step pays one scalar add for the address instead of a
// 64-bit product and a vector add.  The wait for the slot's previous content is the compiler's own: `slot_read`, the value the
// caller has just read from that slot, is an operand.  M0 is still saved and restored inside the statement: the compiler takes
// "m0" in a clobber list only with the remark that a reserved register "may not be preserved across the asm statement".
__device__ __forceinline__ void quad_act_fetch(const int32_t *row, const uint32_t lane_off, const uint32_t lds_slot, const uint32_t slot_read)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(lane_off), "s"(row), "s"(lds_slot), "v"(slot_read) : "memory");
}

// U2 + U4: the action force of index `ai`, one of five constants, with the step's own expressions (so the bits are the step's);
// any index outside 0..4 gives no force.  {u_x + 0, u_y + 0}: the accumulators' starting values.
__device__ __forceinline__ float2 quad_action_force(const int ai, const float sens, const float fscale)
{
    float ux = 0.0f + ((ai == 1 ? 1.0f : 0.0f) - (ai == 2 ? 1.0f : 0.0f));
    float uy = 0.0f + ((ai == 3 ? 1.0f : 0.0f) - (ai == 4 ? 1.0f : 0.0f));
    ux *= sens; uy *= sens;
    if (fscale != 1.0f) { ux = fscale * ux; uy = fscale * uy; }
    return make_float2(ux + 0.0f, uy + 0.0f);
}

// The pair force of a physics lane: pw_common.hpp collision_force_pair<true, K1> behind the near test, with the two tests folded
// into ONE exec region -- fast = near & in_range runs the range-restricted expressions; a near pair out of their range (coincident
// agents, NaN / inf, an exotic margin) is rare enough for a wave-uniform test that falls through, and takes collision_force_pair
// itself in a cold block.  The operations and their operands are collision_force_pair's, so the bits are; only the ORDER differs:
// the division by dist (its reciprocal, its two quotient chains) starts right behind the square root and runs beside the margin
// division and the softplus instead of after them -- it needs nothing of theirs but the final product.
template <bool K1>
__device__ __forceinline__ void quad_pair_force(const float2 qi, const float2 qj, const uint32_t near_lo, const uint32_t near_span,
                                                const float dist_min, const float k, const float cf, float &Fx, float &Fy)
{
    // the near test on (p_i - p_j)^2, the force's own delta, so that the two share their first operations (the other
    // kernels test (p_j - p_i)^2: the same value -- a difference and its negation have the same square): -1.7 % step time
    const float dx = qi.x - qj.x, dy = qi.y - qj.y;
    const float d2 = dx * dx + dy * dy;
    const f32x2 a = {cf * dx, cf * dy};
    const bool near = __float_as_uint(d2) - near_lo >= near_span;  // not provably far (NaN / inf included)
    const bool uni = (k >= 9.094947017729282e-13f) & (k <= 1099511627776.0f) & (cf >= 9.5367431640625e-07f) & (cf <= 128.0f);
    const bool c1 = (__float_as_uint(d2) - 0x12800000u) < (0x6C800000u - 0x12800000u);
    const bool c2 = fminf(fabsf(a.x), fabsf(a.y)) >= 8.673617379884035e-19f;
    const bool fast = near & c1 & c2 & uni;
    // (taken here, beside the compares, the wave's mask is theirs, combined in scalar registers)
    const bool any_cold = __builtin_amdgcn_ballot_w64(near & !fast) != 0;
    Fx = 0.0f; Fy = 0.0f;
    if (fast) {
        const float dist = sqrt_rn_core(d2);
        const float y0 = __builtin_amdgcn_rcpf(dist);
        __builtin_amdgcn_sched_barrier(0);  // the reciprocal is in flight before anything of the softplus chain issues
        const float yd = __builtin_fmaf(__builtin_fmaf(-dist, y0, 1.0f), y0, y0);   // div_refined_rcp(dist)
        const f32x2 Q = div_chain2(a, dist, yd);
        const float xarg = K1 ? div_chain1(-(dist - dist_min), k, div_refined_rcp(k))
                              : div_chain(-(dist - dist_min), k, div_refined_rcp(k));
        const float pen = softplus_branchless(xarg) * k;
        const f32x2 F = Q * f32x2{pen, pen};
        Fx = F.x;
        Fy = F.y;
    }
    if (__builtin_expect(any_cold, 0)) {
        if (near & !fast) collision_force_pair<true, K1>(qi.x, qi.y, qj.x, qj.y, dist_min, k, cf, Fx, Fy);
    }
}

// The collision half of an output lane's step: the six threshold tests of the lane's agent `mine` against its env's agents
// q6[0..5] (the self pair included: d2 = 0 passes, a NaN / inf position fails its own test), their number and, COLL, their
// mask.  Wave OB runs it in every step, wave OA for a launch's last step only -- one body, so the two cannot drift apart.
template <bool COLL>
__device__ __forceinline__ void quad_coll_tests(const float2 mine, const float2 (&q6)[6], const float coll_thr2, int &cnt, uint32_t &cmask)
{
    cnt = 0; cmask = 0;
#if defined(PW_EXPERIMENTS) && defined(PW_EXP_NO_COLL_TESTS)   // tools/experiments/pw_experiments.hpp: a timing-only build, which build_native.py refuses
    cnt = 1;
#else
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const float2 q = q6[j];
        const float dx = q.x - mine.x, dy = q.y - mine.y;
        const float d2 = dx * dx + dy * dy;
        cnt += d2 < coll_thr2 ? 1 : 0;
        if (COLL) cmask |= d2 < coll_thr2 ? 1u << j : 0u;
    }
#endif
}

// COLL: wave OB also stores the step's collision masks (pw_step_io.coll) -- it holds the six threshold tests anyway, so
// the instantiation differs by one mask accumulation and one 8-byte store per lane and step; every other output is
// bit-identical to the plain form (tests: the `quad+coll` path, and the bench-path test at C2 full size).
// K1: the division by the contact margin inside the force runs as ONE Newton correction (pw_common.hpp div_chain1); the
// host sets it only for margins whose refined reciprocal is the correctly rounded one (pworld.hip margin_one_correction).
#ifndef PW_QUAD_BARRIER
#define PW_QUAD_BARRIER(t) duo_barrier()   // one workgroup meeting per step
#endif
#ifndef PW_QUAD_ACT_AHEAD
#define PW_QUAD_ACT_AHEAD 4   // iterations wave OB fetches the action indices ahead of their use (a power of two; slots of its LDS ring)
#endif
#ifndef PW_QUAD_PAD_P   // timing experiments only (tools/experiments/pw_experiments.hpp): padding of a wave's step loop
#define PW_QUAD_PAD_P()
#endif
#ifndef PW_QUAD_PAD_OB
#define PW_QUAD_PAD_OB()
#endif
#ifndef PW_QUAD_RESET_XY   // timing experiments only (PW_EXP_NO_RESET_DRAWS): a wave kind's reset draws; kind 1 physics, 2 OA, 4 OB
#define PW_QUAD_RESET_XY(kind, seed, env_id, episode, entity, x, y) pw_reset_xy(seed, env_id, episode, entity, -1.0f, 1.0f, x, y)
#endif
#ifndef PW_QUAD_DRAW_ROUNDS
#define PW_QUAD_DRAW_ROUNDS 10  // Philox rounds (of each of its two draws) wave OB runs per iteration while it draws ahead: 1, 2, 5 or 10 (measured: 10)
#endif
#ifndef PW_QUAD_DRAW_DELAY
#define PW_QUAD_DRAW_DELAY 1    // iterations behind a reset step at which the first slice runs (>= 1: the reset iteration itself is OB's longest)
#endif
constexpr int kQuadActAhead = PW_QUAD_ACT_AHEAD;
constexpr int kQuadN = 6, kQuadL = 6, kQuadEPP = 4, kQuadEPW = 8;   // agents, landmarks, envs per physics wave / per workgroup
// ------------------------------------------------------------------------------------------
// Reset draws ahead (round 9, profiles/r9_quad_reset_bound.txt, r9_quad_reset_ahead.txt).  A reset position is
// pw_reset_xy(seed, env_id, ep_count + 1, entity): every operand is known when the CURRENT episode begins.  With a fixed episode length all
// envs of a workgroup (of the whole batch) reset in the same step, and in that step each physics lane ran Philox4x32-10 (twenty 64-bit
// products, quarter rate) on the step's critical path, and OA and OB each ran it again for the same 48 landmarks one iteration later.
// Now wave OB, lane (env e, index a), draws BOTH entities a (the agent) and N + a (the landmark it owns) of episode ep_count + 1 ahead, in
// kQuadDrawSlices slices of kQuadDrawRounds Philox rounds of each draw, one slice per iteration, the state in registers (the two chains
// are independent and interleave); the last slice converts and publishes: the agent's position to s_drawA[me], where physics lane `me`
// finds it with one ds_read_b64, the landmark's to s_drawL[me] for OA lane `me`, and OB keeps its own copy in registers.  Same Philox, same
// counters and keys, same float conversion (quad_draw_xy is pw_reset_xy's, tests/quad_draw_rule_dump.hip compares them on the host): the
// bits do not change, only where and when they are made.
// Slice size and start are a MEASURED choice (profiles/r9_quad_reset_ahead.txt, us per step at B = 4096, parent 0.522): 1 round per
// iteration 0.505, 2 rounds 0.495, 5 rounds 0.494, all 10 in ONE iteration 0.488; that one slice 2, 3, 6 iterations behind the reset step
// instead of 1: 0.497, 0.495, 0.496; 5 rounds starting 3 behind: 0.488.  Spreading the quarter-rate products thin does not pay: every
// iteration with a slice in it is a longer iteration of OB's, and one long iteration right behind the reset step -- where the physics
// waves have just waited for OB's longest iteration anyway -- costs least.  So the default is one slice (kQuadDrawSlices = 1, depth 2).
// The pipeline is WORKGROUP-uniform and every wave derives its state from the clocks it follows anyway: it starts in OB's iteration
// t_start = 0 of a launch, or t_start = t + 1 behind a reset step t, and only if all clocks of the workgroup are equal (then every env
// resets in step t_reset) and that reset is at least kQuadDrawDepth steps away (quad_draw_engages); then t_fast = t_reset, else no slice
// is issued and t_fast = -1.  A reset step with t == t_fast is the fast one: the physics lanes and OA read their entry, OB takes its
// registers, t_reset advances by the episode length with one scalar add (no lane reads), and the pipeline restarts.  Every other reset
// step -- clocks apart, episodes shorter than the depth, a launch that begins closer to a reset than the depth, T = 1 -- runs the code
// that was there before.
// Who waits for what (no meeting of its own): the slices run in OB's iterations t_start .. t_start + kQuadDrawSlices - 1, the entries are
// written in the last of them, i.e. between barriers t_start + kQuadDrawSlices - 1 and t_start + kQuadDrawSlices (OB's barrier waits for
// its LDS operations).  t_fast >= t_start + kQuadDrawDepth = t_start + kQuadDrawSlices + 1: a physics lane reads in step t_fast, behind
// barrier t_fast - 1 >= t_start + kQuadDrawSlices; OA reads in its iteration t_fast, behind barrier t_fast.  The entries are written
// again by the NEXT pipeline only (with equal clocks no other reset lies in between), which starts at t_fast + 1 and writes behind barrier
// t_fast + kQuadDrawSlices: the physics lanes arrived at barrier t_fast, and OA at barrier t_fast + 1, with their reads done.
// The entries live in LDS nobody used: ring entries 48..63 of the four slots (a slot holds 8 envs x 6 agents = 48 states; every ring
// access in this file is indexed by a ring index < 48, idle lanes shadowing lane 0).  Entry i of a region: 32 entries in one slot's tail,
// the other 16 in the next slot's (quad_draw_at).
// ------------------------------------------------------------------------------------------
constexpr int kQuadDrawRounds = PW_QUAD_DRAW_ROUNDS, kQuadDrawSlices = 10 / kQuadDrawRounds;
constexpr int kQuadDrawDelay = PW_QUAD_DRAW_DELAY;
constexpr int kQuadDrawDepth = kQuadDrawSlices + 1;   // steps from the pipeline's first slice to the first reset step that may use its draws
static_assert(kQuadDrawRounds * kQuadDrawSlices == 10, "a slice is a whole number of Philox4x32-10's rounds");
static_assert(kQuadDrawDelay >= 1, "the pipeline restarts behind the reset step");
constexpr int kQuadNever = 0x7fffffff;
// THE engage rule (all three wave kinds call it, tests/test_quad_draw_rule.py tabulates it): may a reset step that comes
// `steps_since_start` steps after the pipeline's first slice take its positions from the pipeline?
__host__ __device__ inline bool quad_draw_engages(const int auto_reset, const int max_episode_len, const bool clocks_equal, const int steps_since_start)
{
    return auto_reset != 0 && max_episode_len > 0 && clocks_equal && steps_since_start >= kQuadDrawDepth;
}
__host__ __device__ inline int quad_draw_at(const int i) { return (i >> 5) * (2 * kWave) + (i & 31); }   // float2 index of entry i < 48 in s_drawA / s_drawL
// one round of pw_philox4x32_10 (include/pworld_math.h) on a state kept by the caller; k0, k1: the round's keys
__host__ __device__ inline void quad_philox_round(uint32_t (&c)[4], const uint32_t k0, const uint32_t k1)
{
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1; c[3] = (uint32_t)p0; c[0] = n0; c[2] = n2;
}
// pw_reset_xy's conversion of the first two words, lo = -1, hi = 1 (its expressions, so its bits)
__host__ __device__ inline float2 quad_draw_xy(const uint32_t r0, const uint32_t r1)
{
    const float lo = -1.0f, hi = 1.0f;
    const float span = hi - lo;
    const float u0 = (float)(r0 >> 8) * 5.9604644775390625e-8f;
    const float u1 = (float)(r1 >> 8) * 5.9604644775390625e-8f;
    return make_float2(span * u0 + lo, span * u1 + lo);
}
struct SpreadQuadLds { float4 *s_ring; float2 *s_ftab, *s_lmB, *s_utab, *s_u, *s_drawA, *s_drawL; float *s_min, *s_rew; int32_t *s_act; uint32_t bytes; };
__host__ __device__ inline SpreadQuadLds spread_quad_lds(unsigned char *raw = nullptr)
{
    LdsCursor c{reinterpret_cast<float *>(raw)}; SpreadQuadLds o;
    o.s_ring = c.take<float4>(4 * kWave);                        // [4][64] {px, py, vx, vy}, index e_local * 6 + a
    o.s_drawA = reinterpret_cast<float2 *>(o.s_ring + kQuadEPW * kQuadN);               // alias, the tails of ring slots 0 and 1: [48] agent positions of the next episode, OB -> P (quad_draw_at)
    o.s_drawL = reinterpret_cast<float2 *>(o.s_ring + 2 * kWave + kQuadEPW * kQuadN);   // alias, the tails of ring slots 2 and 3: [48] landmark positions of the next episode, OB -> OA
    o.s_ftab = c.take<float2>(2 * kQuadEPP * kQuadN * kQuadN);   // [2 P waves][24 agents][6 partners]
    o.s_min = c.take<float>(kWave); o.s_rew = c.take<float>(kWave);   // [64] each: OB -> OA, a lane's collision count of even / odd steps (int32)
    o.s_lmB = c.take<float2>(kQuadEPW * kQuadL); o.s_act = c.take<int32_t>(2 * kQuadActAhead * kWave);   // [8 * 6] OB; first half: [4 steps][64] action indices (OB)
    o.s_u = reinterpret_cast<float2 *>(o.s_act + kQuadActAhead * kWave);   // alias, inside s_act's second half: [2 steps][48] action force, OB -> P (768 of its 1024 bytes)
    o.s_utab = c.take<float2>(2 * 8);                            // [8] action force per index (OB; the second eight are unused)
    o.bytes = 4 * c.at; return o;
}
template <bool UNIT_MASS, bool COLL = false, bool K1 = false>
__global__ void __launch_bounds__(4 * kWave) pw_spread_quad_kernel(const StreamParams A, const int T)
{
    constexpr int N = kQuadN, L = kQuadL, D = 16, P2 = 15, EPP = kQuadEPP, EPW = kQuadEPW;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const SpreadQuadLds Y = spread_quad_lds(smem_raw);

    // Roles by wave index, swapped in every other batch of 256 workgroups: the hardware places a workgroup's waves 0..3 on
    // the CU's SIMDs in order, and with two workgroups per CU (B = 4096: 512 workgroups on 256 CUs, workgroup j and j + 256
    // on one CU) equal roles would share a SIMD -- the two physics waves, the step's critical path, competing for issue
    // while two output waves with hundreds of cycles of slack share another.  Swapped, every SIMD holds one physics and one
    // output wave: -2.2 % step time (A/B, profiles/r3_quad_waves.txt).
    const int wave = __builtin_amdgcn_readfirstlane((((int)threadIdx.x >> 6) + 2 * (((int)blockIdx.x >> 8) & 1)) & 3);
    const int lane = (int)threadIdx.x & 63;
    // Measured and NOT kept (profiles/r7_quad_balance.txt): an XCD's env blocks contiguous -- block (j % 8) * (G / 8) + j / 8 for workgroup
    // j, so that neighbouring blocks' pieces of the small output planes (rew 192, rew_shared 32, done 48, terminal 8 bytes per block and
    // step share cache lines) meet in one L2: slower, on this kernel and on its predecessor.
    const int env0 = (int)blockIdx.x * EPW;
    const int envs_here = A.B - env0 < EPW ? A.B - env0 : EPW;
    const size_t BN = (size_t)A.B * N;

    // Episode clocks.  Every wave follows the clocks of all 8 envs (lane e < 8 <-> env e), but not by counting: a clock
    // is kept as an offset -- clock before step t = t + off -- so nothing has to be incremented, and the workgroup-uniform
    // question "does any env reset in this step?" is one scalar compare with t_reset, the first step in which one does;
    // the vector work (which envs, the new offsets, the next t_reset) runs only in those steps.
    const bool resets = A.auto_reset && A.max_episode_len > 0;
    int offs_all = A.ep_step[env0 + (lane < envs_here ? lane : 0)];
    auto next_reset_step = [&](int t_from) -> int {  // first step >= t_from in which some env's clock reaches max_episode_len
        if (!resets) return 0x7fffffff;
        int rem = A.max_episode_len - 1 - (t_from + offs_all);
        rem = rem < 0 ? 0 : rem;
        int m = 0x7fffffff;
        for (int e = 0; e < envs_here; ++e) {  // 8 scalar reads: runs once per episode end
            const int r = __builtin_amdgcn_readlane(rem, e);
            m = r < m ? r : m;
        }
        return t_from + m;
    };
    int t_reset = next_reset_step(0);
    // The draw pipeline's state (see "Reset draws ahead" above): t_fast, the reset step that takes its positions from the pipeline, or -1.
    auto clocks_equal = [&]() -> bool { return __builtin_amdgcn_ballot_w64(offs_all != __builtin_amdgcn_readfirstlane(offs_all)) == 0; };  // (idle lanes hold env 0's)
    int t_fast = quad_draw_engages(A.auto_reset, A.max_episode_len, clocks_equal(), t_reset) ? t_reset : -1;   // first slice in iteration 0
    auto reset_step_update = [&](int t) {  // call in a step with t == t_reset, once: the clocks that reached the end restart; the pipeline restarts behind the step
        if (t == t_fast) {  // every clock restarts: no lane reads
            offs_all = -(t + 1);
            t_reset = t + A.max_episode_len;
            t_fast = quad_draw_engages(A.auto_reset, A.max_episode_len, true, A.max_episode_len - kQuadDrawDelay) ? t_reset : -1;
        } else {
            if (t + 1 + offs_all >= A.max_episode_len) offs_all = -(t + 1);
            t_reset = next_reset_step(t + 1);
            t_fast = quad_draw_engages(A.auto_reset, A.max_episode_len, clocks_equal(), t_reset - (t + kQuadDrawDelay)) ? t_reset : -1;
        }
    };
    int cur = 0;  // ring slot of the current state: workgroup-uniform

    // Measured and NOT kept (round 3, profiles/r3_quad_waves.txt): LDS step counters instead of the per-step s_barrier (the
    // physics waves polling-free, the output waves polling with s_sleep).  With the output waves shortened the barrier costs
    // a physics wave little beyond the LDS wait it needs anyway (its next operands), and the counters' own reads and writes
    // cost more: 0.656 instead of 0.615 us per step.
    if (wave < 2) {
        // ================================ waves P0, P1: pair-parallel physics ================================
        // the physics waves are the step's critical path, the output waves have slack: where one of each shares a SIMD
        // (two workgroups per CU at B = 4096) the arbiter should serve the physics wave first
        __builtin_amdgcn_s_setprio(3);
        const int e0 = wave * EPP;
        const int nv = envs_here - e0 < 0 ? 0 : envs_here - e0 < EPP ? envs_here - e0 : EPP;  // envs of this wave
        if (nv == 0) {  // nothing to advance: keep the workgroup's barriers company
            for (int t = 0; t < T; ++t) PW_QUAD_BARRIER(t);
            return;
        }
        // agent lanes (lane < nv * 6; the others shadow lane 0)
        const int la = lane < nv * N ? lane : 0;
        const int e4 = la / N, a = la - e4 * N;
        const int me = (e0 + e4) * N + a;                       // ring index
        const int env = env0 + e0 + e4;
        const uint32_t g = (uint32_t)env * (uint32_t)N + (uint32_t)a;
        const uint64_t env_id = A.env_id_base + (uint64_t)env;
        // pair lanes (lane < nv * 15; the others shadow pair 0)
        const int lp = lane < nv * P2 ? lane : 0;
        const int pe = lp / P2, pq = lp - pe * P2;
        int pi, pj;
        quad_pair_of(pq, pi, pj);
        const int ri = (e0 + pe) * N + pi, rj = (e0 + pe) * N + pj;
        // force table [agent][partner slot]: a row holds the agent's 5 partners in ascending order (slot = partner index,
        // minus one behind the agent's own index), padded to 6 entries so that rows stay 16-byte aligned
        float2 *ftab = Y.s_ftab + wave * (EPP * N * N);
        float2 *f_ij = ftab + (pe * N + pi) * N + (pj - 1), *f_ji = ftab + (pe * N + pj) * N + pi;   // pi < pj
        const float2 *row = ftab + (e4 * N + a) * N;

        float px = A.pos_x[g], py = A.pos_y[g], vx = A.vel_x[g], vy = A.vel_y[g];
        int ep_off = A.ep_step[env];  // clock before step t = t + ep_off
        uint32_t ep_count = A.ep_count[env];
        Y.s_ring[me] = make_float4(px, py, vx, vy);
        // The action force {u_x + 0, u_y + 0} of step t arrives from wave OB through Y.s_u[t & 1][me], written two steps ahead (see
        // there: who waits for what); the step loop holds no vector memory operation at all.  Steps 0 and 1 have no iteration of OB's
        // in front of them: this wave fetches and decodes those two itself, here, into the same two slots (its own lanes' entries;
        // a launch of one step reads step 0's index twice).
        float2 *u_w = Y.s_u + me;
        {
            const int32_t a0 = A.act[g], a1 = A.act[(T > 1 ? BN : (size_t)0) + g];
            u_w[0] = quad_action_force(a0, A.sens, A.fscale);
            u_w[kQuadEPW * N] = quad_action_force(a1, A.sens, A.fscale);
        }
        int u_at = 0;                 // the entry of the coming step: 0 <-> 48, toggled (a lane's constant offset, nothing selected)
        const float2 *draw_r = Y.s_drawA + quad_draw_at(me);   // this lane's position of the next episode, once wave OB has drawn it
        const float k = A.contact_margin, cf = A.contact_force, dt = A.dt, damp = A.damp, mass = A.mass;
        const uint32_t near_lo = __float_as_uint(A.near_thr2), near_span = 0x7F800000u - near_lo;
        // the pair lanes' operands of the coming step are fetched right after the publish, before the barrier (this
        // wave only reads its own envs' entries, and a wave's LDS operations execute in issue order): the read's latency
        // hides behind the barrier
        float2 qi = *reinterpret_cast<const float2 *>(Y.s_ring + ri);
        float2 qj = *reinterpret_cast<const float2 *>(Y.s_ring + rj);
        PW_STAMP_DECL;
        for (int t = 0; t < T; ++t) {
            PW_STAMP_START;
            const float2 u0 = u_w[u_at];                // consumed behind the pair phase
            u_at = kQuadEPW * N - u_at;
            const bool two_slots = t == t_reset;        // workgroup-uniform: some env of the workgroup resets in this step
            // ---- pair phase: every unordered pair of the wave's envs at once
            float Fx, Fy;
            quad_pair_force<K1>(qi, qj, near_lo, near_span, A.dist_min, k, cf, Fx, Fy);
            *f_ij = make_float2(Fx, Fy);
            *f_ji = make_float2(-Fx, -Fy);
            PW_STAMP(0);
            float fx = u0.x, fy = u0.y;
            asm volatile("" ::: "memory");  // program-order point between table writes and row reads
            // ---- U5: the agent's row, ascending partner order
#pragma unroll
            for (int j = 0; j < N - 1; ++j) {
                const float2 F = row[j];
                fx = F.x + fx;
                fy = F.y + fy;
            }
            // ---- U6
            vx = vx * damp; vy = vy * damp;
            vx = vx + div_mass<UNIT_MASS>(fx, mass) * dt;
            vy = vy + div_mass<UNIT_MASS>(fy, mass) * dt;
            px = px + vx * dt;
            py = py + vy * dt;
            int nxt = (cur + 1) & 3;
            Y.s_ring[nxt * kWave + me] = make_float4(px, py, vx, vy);
            if (__builtin_expect(two_slots, 0)) {  // rare (once per episode): the envs at their episode's end restart, EVERY env publishes a second slot
                const bool fast = t == t_fast;  // workgroup-uniform: every env restarts, at the position wave OB drew ahead
                if (fast || t + 1 + ep_off >= A.max_episode_len) {
                    ep_count += 1;
                    ep_off = -(t + 1);
                    if (fast) {  // written at least one barrier ago (see "Reset draws ahead"): no Philox here
                        const float2 d = *draw_r;
                        px = d.x; py = d.y;
                    } else {
                        PW_QUAD_RESET_XY(1, A.seed, env_id, ep_count, (uint32_t)a, &px, &py);
                    }
                    vx = 0.f; vy = 0.f;
                }
                reset_step_update(t);
                nxt = (nxt + 1) & 3;
                Y.s_ring[nxt * kWave + me] = make_float4(px, py, vx, vy);
            }
            cur = nxt;
            asm volatile("" ::: "memory");
            qi = *reinterpret_cast<const float2 *>(Y.s_ring + cur * kWave + ri);
            qj = *reinterpret_cast<const float2 *>(Y.s_ring + cur * kWave + rj);
            PW_STAMP(1);
            PW_QUAD_PAD_P();
            PW_QUAD_BARRIER(t);
            PW_STAMP(2);
        }
#ifdef PW_STAMPS
        if (blockIdx.x == 0 && wave == 0 && lane == 0)
            for (int i_ = 0; i_ < 4; ++i_) g_pw_stamps[i_] = st_acc[i_];
#endif
        A.pos_x[g] = px; A.pos_y[g] = py;
        A.vel_x[g] = vx; A.vel_y[g] = vy;
        A.ep_step[env] = T + ep_off;
        A.ep_count[env] = ep_count;
        return;
    }

    // ================================ waves OA, OB: outputs of 8 envs, one step behind ================================
    int e_local = lane / N;
    int a = lane - e_local * N;
    if (e_local >= envs_here) { e_local = 0; a = 0; }  // idle lane: shadow lane 0
    const int env = env0 + e_local;
    const int base = e_local * N, me = base + a;
    const uint32_t g = (uint32_t)env * (uint32_t)N + (uint32_t)a;
    const uint64_t env_id = A.env_id_base + (uint64_t)env;
    int ep_off = A.ep_step[env];  // clock before step t = t + ep_off
    uint32_t ep_count = A.ep_count[env];
    float olx = A.lm_x[(size_t)env * L + a], oly = A.lm_y[(size_t)env * L + a];  // the landmark this lane owns

    if (wave == 2) {
        // (round 2 ran this wave at priority 3 too, when it was as long as the physics waves; software-pipelined it has
        // several hundred cycles of slack per step and yields to them)
        // ---------------- OA: masks, rewards, small stores ----------------
        // A step's work has two halves: A(t) -- read the published slot, the owned landmark's minimum over the agents, its
        // sqrt -- and B(t) -- the ordered per-env sums through two rounds of wave shuffles, the stores.  Each half is a chain
        // of long-latency operations (LDS round trips, shuffles, sqrt) with little to issue in between, and B(t) needs
        // nothing but A(t)'s register and the step's collision count: so the loop is software-pipelined, iteration
        // t running B(t - 1) interleaved with A(t) (the shuffles of one fly while the arithmetic of the other issues).
        // Same operations on the same values: the bits do not change.
        // The collision count of step t -- six threshold tests that need nothing this wave owns -- is wave OB's work (it has
        // the issue slots: this wave and OB each share a SIMD with a physics wave of the CU's other workgroup, and the
        // workgroup runs at the pace of the slower pair).  OB leaves it in word `lane` of s_min (t even) / s_rew (t odd)
        // in its iteration t, i.e. before it arrives at barrier t + 1; B(t) reads the word here in iteration t + 1, behind
        // that barrier, and has consumed it before this wave arrives at barrier t + 2; OB writes that buffer again in its
        // iteration t + 2, behind barrier t + 2.  So the hand-over needs no meeting of its own.  Only the launch's last
        // step has no barrier behind it: its count is computed here, after the loop (pre_last: that step's pre-reset slot).
        float own_p = 0.0f;   // A(t - 1): sqrt of the owned landmark's minimum squared distance
        int cnt_p = 0;        // number of agents within the collision threshold in step t - 1 (self included)
        const int *cnt_w = reinterpret_cast<const int *>(Y.s_min) + lane;
        const int cnt_span = (int)(Y.s_rew - Y.s_min);
        int cnt_at = 0;       // word offset of the buffer B(t - 1) reads: 0 <-> cnt_span, workgroup-uniform
        int pre_last = 0;     // the pre-reset slot of the latest A
        const float2 *draw_r = Y.s_drawL + quad_draw_at(me);   // the owned landmark's position of the next episode, once wave OB has drawn it
        // the pieces, in the order an iteration interleaves them
        float2 q6[N];
        auto a_reads = [&](const int nxt) __attribute__((always_inline)) {
            const float4 *slot = Y.s_ring + nxt * kWave + base;
#pragma unroll
            for (int j = 0; j < N; ++j) q6[j] = *reinterpret_cast<const float2 *>(slot + j);
            pre_last = nxt;
        };
        float best, e0;
        auto a_dist = [&]() __attribute__((always_inline)) {
            float e2[N];
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const float2 q = q6[j];
                const float ex = q.x - olx, ey = q.y - oly;
                e2[j] = ex * ex + ey * ey;
            }
            // min() keeps its first argument unless a later one is smaller: a NaN in front stays, NaNs behind are
            // skipped -- i.e. the NaN-ignoring minimum of all six unless the first one is NaN (e2 is never -0): a tree
            best = __builtin_fminf(__builtin_fminf(__builtin_fminf(e2[0], e2[1]), __builtin_fminf(e2[2], e2[3])),
                                   __builtin_fminf(e2[4], e2[5]));
            e0 = e2[0];
        };
        auto a_sqrt = [&]() __attribute__((always_inline)) -> float {
            const float b = e0 != e0 ? e0 : best;
            return sqrtf(b);  // branch-free expansion: the guarded fast form (a vector compare feeding exec) measured 8 % slower on this chain
        };
        auto a_clock = [&](const int t, int nxt) __attribute__((always_inline)) {  // episode clocks; the slot A(t + 1) reads
            if (__builtin_expect(t == t_reset, 0)) {  // workgroup-uniform, once per episode
                const bool fast = t == t_fast;  // workgroup-uniform: every env restarts, with the landmark wave OB drew ahead
                if (fast || t + 1 + ep_off >= A.max_episode_len) {
                    ep_count += 1;
                    ep_off = -(t + 1);
                    if (fast) {
                        const float2 d = *draw_r;
                        olx = d.x; oly = d.y;
                    } else {
                        PW_QUAD_RESET_XY(2, A.seed, env_id, ep_count, (uint32_t)(N + a), &olx, &oly);
                    }
                }
                reset_step_update(t);
                nxt = (nxt + 1) & 3;
            }
            cur = nxt;
        };
        float sh_own[L], sh_r[N], r;
        auto b_shfl_own = [&]() __attribute__((always_inline)) {  // per-env reductions by wave shuffle (ds_bpermute: one trip each, no LDS write -> wait -> read)
#pragma unroll
            for (int l = 0; l < L; ++l) sh_own[l] = __shfl(own_p, base + l, kWave);
        };
        auto b_reward = [&]() __attribute__((always_inline)) {
            r = 0.0f;
#pragma unroll
            for (int l = 0; l < L; ++l) r -= sh_own[l];
            // "rew -= 1" once per colliding agent (itself included): the subtrahends are all the same, so only their
            // number matters; r - 0 is r, so the six steps are selects of the subtrahend, not branches (a loop up to the
            // wave's largest count was measured: a vector compare feeding a scalar branch per iteration costs more)
#pragma unroll
            for (int k2 = 0; k2 < N; ++k2) r -= k2 < cnt_p ? 1.0f : 0.0f;
#pragma unroll
            for (int i = 0; i < N; ++i) sh_r[i] = __shfl(r, base + i, kWave);
        };
        // the planes of step tb: workgroup-uniform running pointers (b_store is called for tb = 0, 1, 2, ... in turn)
        float *rew_t = A.rew, *rsh_t = A.rew_shared;
        auto b_store = [&]() __attribute__((always_inline)) {
            float acc = 0.0f;
#pragma unroll
            for (int i = 0; i < N; ++i) acc += sh_r[i];
            nt_store(rew_t + g, r);
            nt_store(rsh_t + env, acc);   // (done / terminal / coll: wave OB)
            rew_t += BN; rsh_t += A.B;
        };
        PW_STAMP_DECL;
        // prologue: A(0)
        {
            PW_STAMP_START;
            PW_QUAD_BARRIER(0);
            PW_STAMP(0);
            const int nxt = (cur + 1) & 3;
            a_reads(nxt);
            a_dist();
            own_p = a_sqrt();
            a_clock(0, nxt);
            PW_STAMP(1);
        }
        for (int t = 1; t < T; ++t) {  // A(t) interleaved with B(t - 1): no branch but the (rare) reset step's
            PW_STAMP_START;
            PW_QUAD_BARRIER(t);
            PW_STAMP(0);
            const int nxt = (cur + 1) & 3;
            cnt_p = cnt_w[cnt_at];   // step t - 1's count, from wave OB
            cnt_at = cnt_span - cnt_at;
            a_reads(nxt);
            b_shfl_own();
            a_dist();
            b_reward();
            const float own = a_sqrt();
            b_store();
            own_p = own;
            a_clock(t, nxt);
            PW_STAMP(1);
        }
        {   // epilogue: B(T - 1), with the count of this wave's own making (no barrier behind step T - 1; its slot stays as it is:
            // the physics waves have published their last)
            const float4 *slot = Y.s_ring + pre_last * kWave + base;
            const float2 mine = *reinterpret_cast<const float2 *>(slot + a);
#pragma unroll
            for (int j = 0; j < N; ++j) q6[j] = *reinterpret_cast<const float2 *>(slot + j);
            uint32_t cmask;
            quad_coll_tests<false>(mine, q6, A.coll_thr2, cnt_p, cmask);
        }
        b_shfl_own();
        b_reward();
        b_store();
#ifdef PW_STAMPS
        if (blockIdx.x == 0 && lane == 0)
            for (int i_ = 0; i_ < 2; ++i_) g_pw_stamps[4 + i_] = st_acc[i_];
#endif
        return;
    }

    // ---------------- OB: observation rows ----------------
    // The wave's 48 rows are contiguous in the obs plane and are stored as ONE block: 192 chunks of 16 bytes, chunk
    // q = row * 4 + column group, lane l stores chunks l, l + 64, l + 128 -- 1 KiB contiguous per store instruction.
    // With D = 16 a lane's column group c = l & 3 never changes and its rows are l / 4, + 16, + 32: c = 0 is the row's
    // {vel, pos}, c >= 1 the landmarks 2c - 2, 2c - 1 relative to the row's agent (stream_write_obs's subtractions, only
    // the storing lane differs).  The rows' {pos, vel} are read STRAIGHT from the ring slot (its index is the row index),
    // and a lane's three landmark pairs live in registers for the whole episode (they change in reset steps only): a
    // step is three 16-byte LDS reads, the subtractions and three stores.
    // A step's loop body is straight-line code (counted: profiles/r6_quad_loop_census.txt): the three ring reads go out back to
    // back behind ONE wait, column group 0 is composed by selects (no exec-masked region), and no store carries a predicate --
    // in the last, partial workgroup a chunk past the block re-stores chunk `column group` of row 0 instead: the lane reads
    // row 0 and env 0's landmarks, i.e. it computes that chunk's very value, and writes it to that chunk's address (the idiom
    // of the idle lanes' done / terminal / reward stores: a second store of the same bytes).  The output planes are walked by
    // running workgroup-uniform pointers (one 64-bit scalar add per plane and step), the lanes' parts are constant offsets.
    const int rows_here = envs_here * N;
    const int cgrp = lane & 3;
    const bool col0 = cgrp == 0;
    int row_u[3];
    uint32_t off_u[3];  // byte offset of the lane's chunk u in the workgroup's block of a step
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int r = (lane >> 2) + 16 * u;
        const bool ok = r < rows_here;
        row_u[u] = ok ? r : 0;
        off_u[u] = (uint32_t)(ok ? lane + 64 * u : cgrp) * 16u;
    }
    float4 lm_u[3];
    auto load_landmarks = [&]() {  // the two landmarks of this lane's column group, per row's env
#pragma unroll
        for (int u = 0; u < 3; ++u)
            lm_u[u] = *reinterpret_cast<const float4 *>(Y.s_lmB + (row_u[u] / N) * L + (cgrp > 0 ? 2 * cgrp - 2 : 0));
    };
    Y.s_lmB[me] = make_float2(olx, oly);
    // The physics waves' action force is this wave's work too (it has the issue slots, profiles/r6_quad_issue_budget.txt; nothing of it
    // depends on the state): lane l < 48 is ring index `me` = l, the workgroup's 48 indices of a step are contiguous in A.act.  The
    // indices arrive by LDS-direct loads (pw_common.hpp act_fetch_issue: registers rotated through a loop get copied at the back edge, and
    // a copy of a pending load waits for it), step s into slot s & 3 of Y.s_act's first half, fetched kQuadActAhead iterations before
    // they are used; iteration t looks step t + 2's force up in the six-entry table below (entry 5: any index outside 0..4) and writes
    // it to Y.s_u[t & 1][me].  Who waits for what: the write lies between barriers t and t + 1 -- this wave's barrier waits for its LDS
    // operations -- and a physics lane reads the entry at the top of step t + 2, behind barrier t + 1; it has consumed slot t & 1's
    // previous entry (step t's) before it arrives at barrier t, and this wave writes the slot again only behind that barrier.  No
    // meeting of its own.  Steps 0 and 1 are the physics waves' own (see there).  The compiler does not count these loads, but it counts
    // this wave's stores into the same counter, so the wait is written out with the number of vector memory operations a step issues
    // at least: kStepStores stores (a reset step issues more: the wait only gets stricter) and one fetch.  The fetch of step t + 2 was
    // issued kQuadActAhead iterations ago at this place, so kQuadActAhead * kStepStores stores and kQuadActAhead - 1 fetches lie behind
    // it; the fetches issued before the loop, which have fewer behind them, are waited for before the loop (one load's latency at the
    // start of a launch, in the shadow of the physics waves' own start-of-launch loads and first step).  The tail re-fetches the last step: the pointer's stride turns 0 there.
    constexpr int kStepStores = 5 + (COLL ? 1 : 0);   // done, terminal, three observation chunks, the collision mask
    constexpr int kActBehind = kQuadActAhead * kStepStores + kQuadActAhead - 1;
    constexpr int kActWait = kActBehind < 63 ? kActBehind : 63;   // vmcnt is a six-bit field (a smaller count only waits for more)
    const unsigned char *act_row = reinterpret_cast<const unsigned char *>(A.act) + (size_t)(T > 2 ? 2 : T > 0 ? T - 1 : 0) * (BN * sizeof(int32_t));
    const size_t act_stride = BN * sizeof(int32_t);
    const uint32_t act_off = g * (uint32_t)sizeof(int32_t);
    const unsigned char *act_ring = reinterpret_cast<const unsigned char *>(Y.s_act + lane);
    uint32_t act_lds = __builtin_amdgcn_readfirstlane((uint32_t)reinterpret_cast<uintptr_t>(Y.s_act));
    asm volatile("" : "+s"(act_lds));   // (the address as a value of the loop's: otherwise the pointer's null test is repeated in every step)
    constexpr uint32_t kSlotBytes = kWave * sizeof(int32_t), kRingMask = kQuadActAhead * kSlotBytes - 1;
    auto fetch_act = [&](int s, uint32_t slot_at, uint32_t slot_read) {   // indices of step s -> slot s & 3, at byte slot_at of the ring; called for s = 2, 3, 4, ... in turn
        quad_act_fetch(reinterpret_cast<const int32_t *>(act_row), act_off, act_lds + slot_at, slot_read);
        act_row += s + 1 < T ? act_stride : (size_t)0;
    };
    // every load the compiler counts is consumed before the first uncounted one is issued: a counted wait inside the loop (for a
    // value first used there, as ep_count in a reset step) would be short by the fetches in flight, i.e. drain them
    asm volatile("" :: "v"(ep_off), "v"(ep_count), "v"(offs_all), "v"(olx), "v"(oly), "s"(t_reset));
    // The draws of the next episode (see "Reset draws ahead" above): the two Philox states of this lane, slice t - t_draw in iteration t.
    uint32_t ca[4], cl[4];
    float2 nlm = make_float2(0.0f, 0.0f);   // the finished landmark draw, this wave's own copy
    const uint32_t seed_lo = (uint32_t)A.seed, seed_hi = (uint32_t)(A.seed >> 32);
    float2 *draw_wa = Y.s_drawA + quad_draw_at(me), *draw_wl = Y.s_drawL + quad_draw_at(me);
    int t_draw = kQuadNever;   // the iteration of the pipeline's first slice: workgroup-uniform
    auto draw_start = [&](int t_first) __attribute__((always_inline)) {   // call with ep_count of the episode that runs in iteration t_first
        const bool go = t_fast >= 0;
        t_draw = go ? t_first : kQuadNever;
        ca[0] = (uint32_t)a; cl[0] = (uint32_t)(N + a);
        ca[1] = cl[1] = ep_count + 1u;
        ca[2] = cl[2] = (uint32_t)env_id;
        ca[3] = cl[3] = (uint32_t)(env_id >> 32);
    };
    draw_start(0);
    for (int s0 = 2; s0 < 2 + kQuadActAhead; ++s0) fetch_act(s0, ((uint32_t)s0 * kSlotBytes) & kRingMask, 0u);
    if (lane < 6) Y.s_utab[lane] = quad_action_force(lane, A.sens, A.fscale);
    float2 *u_w = Y.s_u + me;
    int u_at = 0;             // the entry iteration t writes: 0 <-> 48, toggled
    uint32_t act_slot = (2 * kSlotBytes) & kRingMask;   // byte offset of slot (t + 2) & 3
    wave_lds_sync();
    load_landmarks();
    act_fetch_drain();
    // workgroup-uniform plane pointers of step t (the compiler keeps them in scalar registers: every term is uniform)
    unsigned char *obs_t = reinterpret_cast<unsigned char *>(A.obs + ((size_t)env0 * N) * D);
    uint8_t *done_t = A.done, *term_t = A.terminal;
    const size_t obs_stride = BN * D * sizeof(float);
    // the terminal flag of step t is "t >= t_term": t + 1 + ep_off >= max_episode_len, solved for t (changes in reset steps only)
    const bool has_len = A.max_episode_len > 0;
    int t_term = has_len ? A.max_episode_len - 1 - ep_off : 0x7fffffff;
    // The collision half of wave OA's step runs here (see there: who waits for what): in every step this lane -- in its (env, agent)
    // mapping, idle lanes shadowing lane 0 -- tests its agent against the env's six in the PRE-reset slot, the slot OA's A(t) reads,
    // and leaves the count in word `lane` of s_min / s_rew (even / odd steps; the offset toggles, nothing is selected).  COLL: the
    // step's mask plane leaves from here as well.  Straight-line: seven broadcast reads, selects, one LDS write.
    int *cnt_w = reinterpret_cast<int *>(Y.s_min) + lane;
    const int cnt_span = (int)(Y.s_rew - Y.s_min);
    int cnt_at = 0;
    uint64_t *coll_t = A.coll;
    PW_STAMP_DECL;
    for (int t = 0; t < T; ++t) {
        PW_STAMP_START;
        nt_store(done_t + g, (uint8_t)0);
        PW_QUAD_BARRIER(t);
        PW_STAMP(0);
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(kActWait) : "memory");  // step t + 2's indices are in LDS (the later fetches and this wave's recent stores stay in flight)
        const uint32_t ai = *reinterpret_cast<const uint32_t *>(act_ring + act_slot);
        int nxt = (cur + 1) & 3;
        float2 cmine, cq6[N];
        {
            const float4 *pre = Y.s_ring + nxt * kWave + base;
            cmine = *reinterpret_cast<const float2 *>(pre + a);
#pragma unroll
            for (int j = 0; j < N; ++j) cq6[j] = *reinterpret_cast<const float2 *>(pre + j);
        }
        fetch_act(t + 2 + kQuadActAhead, act_slot, ai);  // into the slot just read (its wait for the read above is the one the table lookup needs anyway)
        act_slot = (act_slot + kSlotBytes) & kRingMask;
        const float2 u2 = Y.s_utab[ai < 5u ? ai : 5u];
        nt_store(term_t + env, (uint8_t)(t >= t_term ? 1 : 0));
        if (t == t_reset) {  // workgroup-uniform, once per episode
            const bool rst = t >= t_term;
            if (rst) {
                if (A.final_obs) {
                    const float4 st = Y.s_ring[nxt * kWave + me];  // this lane's own (env, agent) row, pre-reset
                    stream_write_obs<L>(A.final_obs + ((size_t)t * BN + g) * D, L, Y.s_lmB + base, st.x, st.y, st.z, st.w);
                }
                ep_count += 1;
                ep_off = -(t + 1);
                t_term = A.max_episode_len - 1 - ep_off;
                if (t == t_fast) { olx = nlm.x; oly = nlm.y; }   // workgroup-uniform: every env restarts, with the landmark drawn ahead
                else PW_QUAD_RESET_XY(4, A.seed, env_id, ep_count, (uint32_t)(N + a), &olx, &oly);
            }
            reset_step_update(t);
            draw_start(t + kQuadDrawDelay);
            wave_lds_sync();     // the pre-reset rows have read the old landmarks
            if (rst) Y.s_lmB[me] = make_float2(olx, oly);
            wave_lds_sync();
            load_landmarks();
            nxt = (nxt + 1) & 3;  // the post-reset slot (the same state for envs that did not reset)
        }
        cur = nxt;
        const float4 *slot = Y.s_ring + nxt * kWave;
        float4 st[3];
#pragma unroll
        for (int u = 0; u < 3; ++u) st[u] = slot[row_u[u]];
        {   // (the tests' operands were read first: they run while the rows arrive)
            int cnt;
            uint32_t cmask;
            quad_coll_tests<COLL>(cmine, cq6, A.coll_thr2, cnt, cmask);
            cnt_w[cnt_at] = cnt;   // complete before this wave arrives at the next barrier (its s_waitcnt)
            cnt_at = cnt_span - cnt_at;
            u_w[u_at] = u2;        // step t + 2's action force, likewise complete before the next barrier
            u_at = kQuadEPW * N - u_at;
            if (COLL) {
                nt_store(coll_t + g, (uint64_t)cmask);   // is_collision bits of the state step t produced (pre-reset)
                coll_t += BN;
            }
        }
        // anchor: the rows arrive whole behind one wait (otherwise the compiler splits row 0's read between the two sides of an
        // exec-masked region it makes of the selects)
        asm volatile("" :: "v"(st[0].x), "v"(st[0].y), "v"(st[0].z), "v"(st[0].w), "v"(st[1].x), "v"(st[1].y), "v"(st[1].z),
                           "v"(st[1].w), "v"(st[2].x), "v"(st[2].y), "v"(st[2].z), "v"(st[2].w));
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const float4 d = make_float4(lm_u[u].x - st[u].x, lm_u[u].y - st[u].y, lm_u[u].z - st[u].x, lm_u[u].w - st[u].y);
            const float4 o = make_float4(col0 ? st[u].z : d.x, col0 ? st[u].w : d.y, col0 ? st[u].x : d.z, col0 ? st[u].y : d.w);
            nt_store(reinterpret_cast<float4 *>(obs_t + off_u[u]), o);
        }
        obs_t += obs_stride; done_t += BN; term_t += A.B;
        const int ph = t - t_draw;   // the pipeline's slice of this iteration; one scalar compare and branch in the steps without
        if ((unsigned)ph < (unsigned)kQuadDrawSlices) {
            uint32_t k0 = seed_lo + (uint32_t)(ph * kQuadDrawRounds) * 0x9E3779B9u, k1 = seed_hi + (uint32_t)(ph * kQuadDrawRounds) * 0xBB67AE85u;
#pragma unroll
            for (int r = 0; r < kQuadDrawRounds; ++r) {
                quad_philox_round(ca, k0, k1);
                quad_philox_round(cl, k0, k1);
                k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
            }
            if (ph == kQuadDrawSlices - 1) {  // done: published before this wave arrives at the next barrier (its s_waitcnt)
                nlm = quad_draw_xy(cl[0], cl[1]);
                *draw_wa = quad_draw_xy(ca[0], ca[1]);
                *draw_wl = nlm;
            }
        }
        PW_QUAD_PAD_OB();
        PW_STAMP(1);
    }
#ifdef PW_STAMPS
    if (blockIdx.x == 0 && lane == 0)
        for (int i_ = 0; i_ < 2; ++i_) g_pw_stamps[6 + i_] = st_acc[i_];
#endif
    A.lm_x[(size_t)env * L + a] = olx;
    A.lm_y[(size_t)env * L + a] = oly;
    act_fetch_drain();  // the tail's fetches have landed before the wave ends
}

}  // namespace
