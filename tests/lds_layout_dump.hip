// Host-only program of tests/test_lds_layout.py: prints, for every kernel family's LDS layout function and every shape its host
// dispatcher admits, one line
//     <layout> <shape>\t<bytes>\t<name:align:alias,...>\t<offset size offset size ...>
// The layout functions return typed pointers into the base they are given: here a static buffer, so an offset is pointer - buffer.
// `size` and `align` are stated HERE, from what the kernel reads and writes in the region (align: 16 for float4 accesses and
// LDS-direct load targets, 8 for float2 / double / uint64_t, 4 otherwise); the offsets and the total are the layout function's.
// An alias region overlaps another one on purpose.  Build: hipcc --offload-host-only -std=c++17 -I csrc -I include.
#include <cstdio>
#include <set>
#include <string>

#include "pw_kernels_generic.hpp"
#include "pw_kernels_spread_quad.hpp"
#include "pw_kernels_tag.hpp"
#include "pw_kernels_policy3j.hpp"
#include "pw_kernels_policy_tag.hpp"
#include "pw_kernels_policy_ref.hpp"
#include "pw_kernels_critic.hpp"

namespace {

constexpr uint32_t kLdsMax = 160 * 1024;   // what the dispatchers admit (PW_LDS_OPTIN)
alignas(16) unsigned char g_lds[4 << 20];    // larger than any layout the loops below form (those past kLdsMax are formed, then dropped)

struct Line {
    std::string sig, nums;
    void r(const char *name, const void *ptr, size_t size, int align, bool alias = false)
    {
        const size_t off = static_cast<const unsigned char *>(ptr) - g_lds;
        sig += (sig.empty() ? "" : ",") + std::string(name) + ":" + std::to_string(align) + ":" + (alias ? "1" : "0");
        nums += (nums.empty() ? "" : " ") + std::to_string(off) + " " + std::to_string(size);
    }
    void print(const char *key, uint32_t bytes) const { std::printf("%s\t%u\t%s\t%s\n", key, bytes, sig.c_str(), nums.c_str()); }
};

void actor16_regions(Line &l, const Actor16Lds &o, int N, int rows, int S1)
{
    l.r("xf", o.s_xf, (size_t)N * 4096, 16);
    l.r("hx", o.s_hx, 8192, 16);
    l.r("hf", o.s_hf, (size_t)((rows + 15) / 16) * 4096, 16);
    l.r("f_w1", o.f_w1, (size_t)2 * S1 * 64 * 4, 16);
    l.r("b1", o.s_b1, 256, 4);
}

int tag_obs_dim(int N, int A, int L) { return 4 + 2 * L + 2 * (N - 1) + 2 * (A > 0 ? N - A : N - A - 1); }

void env_layouts()
{
    char key[128];
    std::set<std::string> seen;
    for (int N = 1; N <= PW_MAX_AGENTS; ++N)
        for (int epw = 1; epw <= kWave / N; ++epw)
            for (int L = 0; L <= PW_MAX_LANDMARKS; ++L) {
                const size_t nl = (size_t)epw * N, ll = (size_t)epw * L;
                {
                    const Smem o = smem_lds(epw, N, L, g_lds);
                    Line l;
                    l.r("pos", o.pos, nl * 8, 8); l.r("vel", o.vel, nl * 8, 8); l.r("lm", o.lm, ll * 8, 8); l.r("red", o.red, ll * 4, 4);
                    std::snprintf(key, sizeof key, "env_generic N=%d L=%d epw=%d", N, L, epw);
                    l.print(key, o.bytes);
                }
                {
                    const TagStreamLds o = tag_stream_lds(epw, L, g_lds);
                    Line l;
                    l.r("pos", o.s_pos, 512, 8); l.r("vel", o.s_vel, 512, 8); l.r("mlo", o.s_mlo, 256, 4); l.r("mhi", o.s_mhi, 256, 4);
                    l.r("rew", o.s_rew, 256, 4); l.r("lm", o.s_lm, ll * 8, 8);
                    std::snprintf(key, sizeof key, "tag_stream N=%d L=%d epw=%d", N, L, epw);
                    l.print(key, o.bytes);
                }
                // pw_tag_duo_kernel: no observation blocks, and both chunk widths for every row length D <= 32 some roster has
                for (int A = -1; A <= N; ++A)
                    for (int blk = A < 0 ? 0 : 2; blk <= (A < 0 ? 0 : 4); blk += 2) {
                        const int D = A < 0 ? 0 : tag_obs_dim(N, A, L);
                        if (blk && (D > 32 || D < 2)) continue;
                        if (blk == 4 && (nl * D) % 4 != 0) continue;
                        std::snprintf(key, sizeof key, "tag_duo N=%d L=%d epw=%d blk=%d D=%d", N, L, epw, blk, D);
                        if (!seen.insert(key).second) continue;
                        const TagDuoLds o = tag_duo_lds(epw, L, D, g_lds);
                        Line l;
                        l.r("ring", o.s_ring, 3072, 16); l.r("mlo", o.s_mlo, 256, 4); l.r("mhi", o.s_mhi, 256, 4); l.r("rew", o.s_rew, 256, 4);
                        l.r("lm_p", o.s_lm_p, ll * 8, 8); l.r("lm_o", o.s_lm_o, ll * 8, 8); l.r("act", o.s_act, 4 * kWave * 4, 16);
                        l.r("rows", o.s_rows, (size_t)kWave * D * 4, 16);
                        // the compile-time rosters (N, A, L) = (6, 4, 2) and (4, 3, 2) compose the block from {state, zero} instead
                        if (blk && L == 2 && ((N == 6 && D == 22) || (N == 4 && D == 16))) {
                            l.r("state", o.s_state, 1024, 16, true); l.r("zero", o.s_zero, 8, 8, true);
                        }
                        l.print(key, o.bytes);
                    }
                if (L > N) continue;   // the simple_spread fast path: L <= N
                {
                    const SpreadStreamLds o = spread_stream_lds(epw, L, g_lds);
                    Line l;
                    l.r("pos", o.s_pos, 512, 8); l.r("row", o.s_row, 1024, 16); l.r("lm", o.s_lm, ll * 8, 8);
                    std::snprintf(key, sizeof key, "spread_stream N=%d L=%d epw=%d", N, L, epw);
                    l.print(key, o.bytes);
                }
                {
                    const SpreadDuoLds o = spread_duo_lds(epw, L, g_lds);
                    Line l;
                    l.r("ring", o.s_ring, 3072, 16); l.r("lm", o.s_lm, ll * 8, 8); l.r("min", o.s_min, 256, 4); l.r("rew", o.s_rew, 256, 4);
                    l.r("row", o.s_row, 1024, 16); l.r("utab", o.s_utab, 64, 8); l.r("zero", o.s_zero, 8, 8); l.r("actr", o.s_actr, 4 * kWave * 4, 16);
                    std::snprintf(key, sizeof key, "spread_duo N=%d L=%d epw=%d", N, L, epw);
                    l.print(key, o.bytes);
                }
            }
    {
        const SpreadQuadLds o = spread_quad_lds(g_lds);
        Line l;
        l.r("ring", o.s_ring, 4096, 16); l.r("ftab", o.s_ftab, 2 * 4 * 6 * 6 * 8, 8); l.r("min", o.s_min, 256, 4); l.r("rew", o.s_rew, 256, 4);
        l.r("lmB", o.s_lmB, 8 * 6 * 8, 16); l.r("act", o.s_act, 2 * kQuadActAhead * kWave * 4, 16); l.r("utab", o.s_utab, 128, 8);
        l.print("spread_quad", o.bytes);
    }
}

void actor_layouts()
{
    char key[128];
    for (int S1C = 1; S1C <= 8; ++S1C) {
        const int S1 = 4 * S1C;
        {
            const ActorFrontLds o = actor_front_lds(S1, g_lds);
            Line l;
            l.r("f_wih", o.f_wih, 8 * 2 * 4 * 64 * 16, 16); l.r("f_w1", o.f_w1, (size_t)2 * S1 * 64 * 4, 16); l.r("b1", o.s_b1, 256, 4);
            l.r("bih", o.s_bih, 1024, 4); l.r("t", o.s_t, 4 * 32 * 33 * 4, 4);
            std::snprintf(key, sizeof key, "actor_front S1=%d", S1);
            l.print(key, o.bytes);
        }
        {
            const ActorLds o = actor_lds(S1, g_lds);
            Line l;
            l.r("f_wih", o.f_wih, 4 * 2 * 4 * 64 * 16, 16); l.r("whh", o.s_whh, 4 * 8 * 32 * 16, 16); l.r("f_w1", o.f_w1, (size_t)2 * S1 * 64 * 4, 16);
            l.r("g", o.s_g, kFusedRows * kGs * 4, 4); l.r("hid", o.s_hid, kFusedRows * kHs * 4, 16); l.r("b1", o.s_b1, 256, 4);
            l.r("bih", o.s_bih, 1024, 4); l.r("w2", o.s_w2, 4096, 16); l.r("b2", o.s_b2, 64, 4); l.r("hx", o.s_hx, 2048, 16);
            l.r("lg", o.s_lg, kFusedRows * 16 * 4, 4, true);
            std::snprintf(key, sizeof key, "actor_fused S1=%d", S1);
            l.print(key, o.bytes);
        }
        for (int N = 1; N <= 16; ++N) {   // pw_actor_fused: 16 environments per workgroup
            const Actor16Lds o = actor16_lds(N, 16 * N, S1, g_lds);
            if (o.bytes > kLdsMax) continue;
            Line l;
            actor16_regions(l, o, N, 16 * N, S1);
            std::snprintf(key, sizeof key, "actor16 N=%d rows=%d S1=%d", N, 16 * N, S1);
            l.print(key, o.bytes);
        }
    }
}

void rollout_layouts()
{
    char key[128];
    std::set<std::string> seen3j;
    for (int N = 1; N <= PW_MAX_AGENTS; ++N)
        for (int L = 0; L <= N && 4 + 2 * L <= 104; ++L)
            for (int E = 1; E <= 16; ++E) {
                const int D = 4 + 2 * L, S1 = 4 * ((D + 7) / 8), rows3 = E * N;
                const Roll3Lds o = roll3_lds(E, N, L, D, S1, g_lds);
                if (D <= 64 && o.bytes <= kLdsMax) {
                    Line l;
                    actor16_regions(l, Actor16Lds{o.s_xf, o.s_hx, o.s_hf, o.f_w1, o.s_b1, nullptr, 0}, N, rows3, S1);
                    l.r("b2", o.s_b2, 64, 4); l.r("noise", o.s_noise, (size_t)rows3 * 5 * 4, 4); l.r("obs", o.s_obs, (size_t)rows3 * (D + 2) * 4, 8);
                    l.r("act", o.s_act, (size_t)rows3 * 4, 4); l.r("posb", o.s_posb, 8 * kWave * 8, 8); l.r("lmb", o.s_lmb, (size_t)E * L * 8, 8);
                    l.r("fs", o.s_fs, 128, 8); l.r("fc", o.s_fc, 64, 4); l.r("red", o.red, 8192, 8, true);
                    std::snprintf(key, sizeof key, "roll3 E=%d N=%d L=%d D=%d S1=%d", E, N, L, D, S1);
                    l.print(key, o.bytes);
                }
                for (int NP = N; NP <= (N | 1); ++NP)
                    for (int half = 0; half < 2; ++half) {
                        if (!half && (E > 8 * (kWave / N) || D > 64)) continue;   // full head: one slot per environment wave, rows of <= 64 numbers
                        const Roll3jLds j = roll3j_lds(E, NP, L, half != 0, g_lds);
                        std::snprintf(key, sizeof key, "roll3j E=%d NP=%d L=%d half=%d", E, NP, L, half);
                        if (j.bytes > kLdsMax || !seen3j.insert(key).second) continue;   // (NP = N | 1 of an even N is the next N's own)
                        const size_t rows = (size_t)E * NP;
                        Line l;
                        l.r("xf", j.s_xf, 16384, 16); l.r("hx", j.s_hx, 8192, 16);
                        l.r("hf", j.s_hf, half ? (size_t)NP * 2048 : ((rows + 15) / 16) * 4096, 16);
                        l.r("b2", j.s_b2, 64, 4); l.r("st", j.s_st, rows * 16, 16); l.r("act", j.s_act, rows, 1, !half);
                        if (half) l.r("near", j.s_near, rows * 8, 8);
                        l.r("posb", j.s_posb, 8 * kWave * 8, 8); l.r("lmb", j.s_lmb, (size_t)E * L * 8, 8); l.r("fs", j.s_fs, 128, 8);
                        l.r("fc", j.s_fc, 64, 4); l.r("eps", j.s_eps, 64, 4); l.r("epc", j.s_epc, 64, 4); l.r("ret", j.s_ret, 64, 4);
                        l.r("red", j.red, 8192, 8, true);
                        l.print(key, j.bytes);
                    }
            }
    std::set<std::string> seen;
    for (int N = 1; N <= PW_MAX_AGENTS; ++N)   // simple_tag: E = min(96 / N, 16), 9 <= D <= 48
        for (int A = 0; A <= N; ++A)
            for (int L = 0; L <= PW_MAX_LANDMARKS; ++L) {
                const int D = tag_obs_dim(N, A, L), S1C = (D + 7) / 8, E = 96 / N < 16 ? 96 / N : 16;
                if (S1C < 2 || S1C > 6) continue;
                const PolicyTagLds o = policy_tag_lds(4 * S1C, D, E, L, N, g_lds);
                std::snprintf(key, sizeof key, "policy_tag S1=%d D=%d E=%d L=%d N=%d", 4 * S1C, D, E, L, N);
                if (o.bytes > kLdsMax || !seen.insert(key).second) continue;
                Line l;
                actor16_regions(l, o.a16, N, E * N, 4 * S1C);
                l.r("obs", o.s_obs, (size_t)kFusedRows * D * 4, 8); l.r("act", o.s_act, kFusedRows * 4, 4); l.r("posb", o.s_posb, 1024, 8);
                l.r("velb", o.s_velb, 1024, 8); l.r("lmb", o.s_lmb, (size_t)E * L * 8, 8); l.r("mlob", o.s_mlob, 512, 4); l.r("mhib", o.s_mhib, 512, 4);
                l.r("rewb", o.s_rewb, 512, 4); l.r("fs", o.s_fs, 128, 8); l.r("fc", o.s_fc, 64, 4); l.r("noise", o.s_noise, kFusedRows * 2 * 16, 16);
                l.r("red", o.red, 8192, 8, true);
                l.print(key, o.bytes);
            }
    for (int L = 1; L <= 3; ++L) {   // simple_reference: N = 2, 16 environments, D = 2 + 2 L + 3 + dim_c
        const int D = 2 + 2 * L + 3 + kDimC, S1 = 4 * ((D + 7) / 8);
        const PolicyRefLds o = policy_ref_lds(S1, D, 16, g_lds);
        Line l;
        actor16_regions(l, o.a16, 2, 32, S1);
        l.r("obs2", o.s_obs2, (size_t)2 * kFusedRows * D * 4, 4); l.r("act", o.s_act, 2 * kFusedRows * 4, 4); l.r("fs", o.s_fs, 128, 8);
        l.r("fc", o.s_fc, 64, 4); l.r("noise", o.s_noise, 32 * 4 * 16, 16); l.r("red", o.red, 8192, 8, true);
        std::snprintf(key, sizeof key, "policy_ref S1=%d D=%d", S1, D);
        l.print(key, o.bytes);
    }
    for (int N = 1; N <= PW_MAX_AGENTS; ++N) {   // pw_critic_forward: R rows per workgroup by N
        const int R = N <= 32 ? 16 : 8;
        const CriticLds o = critic_lds(N, R, g_lds);
        Line l;
        l.r("out", o.s_out, (size_t)N * 16 * R * 16, 16); l.r("x", o.s_x, (size_t)64 * R * 16, 16); l.r("sc", o.s_sc, (size_t)N * 64, 4);
        l.r("red", o.s_red, 512, 4);
        std::snprintf(key, sizeof key, "critic N=%d R=%d", N, R);
        l.print(key, o.bytes);
    }
}

}  // namespace

int main()
{
    env_layouts();
    actor_layouts();
    rollout_layouts();
    return 0;
}
