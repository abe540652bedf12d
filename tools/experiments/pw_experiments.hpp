// pw_experiments.hpp -- TIMING-ONLY overlays of the product kernels.  NOT part of libpworld.so: this file lives under tools/, the
// product headers include it only under -DPW_EXPERIMENTS (a flag multiagent_rl_amd/build_native.py never passes), and every
// switch below makes the kernels compute WRONG results on purpose -- they bound what a change of schedule could gain before anyone
// builds it.  Build e.g.:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt \
//         -DPW_EXPERIMENTS -DPW_EXP_NO_FORCE -I include -I tools/experiments tools/step_time.hip -o tools/step_time_noforce.bin
// Switches (results: profiles/r4_n3_pair_bound.txt, profiles/r4_c2_bounds.txt):
//   PW_EXP_NO_NT_STORES   outputs that leave through nt_store are computed (kept alive by an empty asm) but not stored: what the
//                         write stream costs a kernel
//   PW_EXP_NO_FORCE       near_force_loop sees an empty near mask: a step without any contact force
//   PW_EXP_ONE_PARTNER    ... with at most ONE evaluation per lane (the bound of a pair-parallel form's gain)
//   PW_EXP_BARRIER2 / 0   the quad kernel's workgroup meets every SECOND step only / never
//   PW_EXP_PAD_OB=<n>     n x `s_nop 0` in the step loop of the quad kernel's wave OB (the results stay right; an experiment build all the
//   PW_EXP_PAD_P=<n>      same) / of its physics waves: does a step pay for every instruction a SIMD issues, or only for the physics
//                         wave's dependent chain?  (profiles/r6_quad_issue_budget.txt)
//   PW_EXP_NO_COLL_TESTS  the quad kernel's six collision tests per output lane and step compiled out, the count fixed at 1 (read by
//                         pw_kernels_spread_quad.hpp quad_coll_tests): the bound of taking that work off a SIMD altogether.  Measured
//                         on the kernel whose wave OA still held the tests (profiles/r7_quad_balance.txt); now they are wave OB's
//   PW_EXP_NO_RESET_DRAWS=<mask>  the quad kernel's reset draws (pw_reset_xy: Philox4x32-10, twenty 64-bit products) replaced by a short
//                         hash of the same operands, per wave kind: bit 0 the physics waves, bit 1 wave OA, bit 2 wave OB (1: P only,
//                         6: OA + OB, 7: all).  What the draws cost a reset step, and whose share reaches the step time
//                         (profiles/r9_quad_reset_bound.txt)
//   (PW_QUAD_ACT_AHEAD=8|16 is a plain parameter of pw_kernels_spread_quad.hpp, not an experiment: results stay exact)
#pragma once
#ifndef PW_EXPERIMENTS
#error "pw_experiments.hpp is a timing-only overlay: compile with -DPW_EXPERIMENTS (never for libpworld.so)"
#endif
#warning "PW_EXPERIMENTS build: kernels may compute WRONG results by design (timing only)"

#if defined(PW_EXP_NO_NT_STORES)
#define PW_HAVE_EXP_NT_STORE 1
template <typename T>
__device__ __forceinline__ void nt_store(T *p, const T v)
{
    if constexpr (sizeof(T) == 8) {
        const unsigned long long u = (unsigned long long)v;
        asm volatile("" :: "v"(p), "v"((unsigned)u), "v"((unsigned)(u >> 32)));
    } else if constexpr (sizeof(T) < 4) {
        asm volatile("" :: "v"(p), "v"((unsigned)v));
    } else {
        asm volatile("" :: "v"(p), "v"(v));
    }
}
__device__ __forceinline__ void nt_store(float4 *p, const float4 v) { asm volatile("" :: "v"(p), "v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w)); }
__device__ __forceinline__ void nt_store(float2 *p, const float2 v) { asm volatile("" :: "v"(p), "v"(v.x), "v"(v.y)); }
#endif

#if defined(PW_EXP_NO_FORCE)
#define PW_NEAR_MASK_HOOK(m) do { (m) = 0; } while (0)
#elif defined(PW_EXP_ONE_PARTNER)
#define PW_NEAR_MASK_HOOK(m) do { (m) &= (decltype(m))0 - (m); } while (0)
#endif

#if defined(PW_EXP_BARRIER2)
#define PW_QUAD_BARRIER(t) do { if (!((t) & 1)) duo_barrier(); else wave_lds_sync(); } while (0)
#elif defined(PW_EXP_BARRIER0)
#define PW_QUAD_BARRIER(t) wave_lds_sync()
#endif

#if defined(PW_EXP_NO_RESET_DRAWS) && PW_EXP_NO_RESET_DRAWS > 0
// kind: 1 physics, 2 OA, 4 OB.  The stand-in must keep the agents' positions independent and uniform on [-1, 1): the physics waves skip
// the force block when no pair of the wave is near, so the contact rate IS the step time (a first stand-in that lined an env's agents
// up 0.25 apart made the step 6 % SLOWER).  Hence a full 32-bit mix: five 32-bit products instead of twenty 64-bit ones.
#define PW_QUAD_RESET_XY(kind, seed, env_id, episode, entity, x, y)                                                              \
    do {                                                                                                                         \
        if ((PW_EXP_NO_RESET_DRAWS) & (kind)) {                                                                                  \
            uint32_t h_ = (uint32_t)(env_id) * 0x9E3779B9u + (episode) * 0x85EBCA6Bu + (entity) * 0xC2B2AE35u + (uint32_t)(seed); \
            h_ ^= h_ >> 16; h_ *= 0x85EBCA6Bu; h_ ^= h_ >> 13; h_ *= 0xC2B2AE35u; h_ ^= h_ >> 16;                                \
            *(x) = 2.0f * ((float)(h_ & 0xFFFFu) * 1.52587890625e-05f) + -1.0f;                                                  \
            *(y) = 2.0f * ((float)(h_ >> 16) * 1.52587890625e-05f) + -1.0f;                                                      \
        } else {                                                                                                                 \
            pw_reset_xy(seed, env_id, episode, entity, -1.0f, 1.0f, x, y);                                                       \
        }                                                                                                                        \
    } while (0)
#endif

#define PW_EXP_STR_(x) #x
#define PW_EXP_STR(x) PW_EXP_STR_(x)
#if defined(PW_EXP_PAD_OB) && PW_EXP_PAD_OB > 0
#define PW_QUAD_PAD_OB() asm volatile(".rept " PW_EXP_STR(PW_EXP_PAD_OB) "\n\ts_nop 0\n\t.endr")
#endif
#if defined(PW_EXP_PAD_P) && PW_EXP_PAD_P > 0
#define PW_QUAD_PAD_P() asm volatile(".rept " PW_EXP_STR(PW_EXP_PAD_P) "\n\ts_nop 0\n\t.endr")
#endif
