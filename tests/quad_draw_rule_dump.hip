// Host-only program of tests/test_quad_draw_rule.py (in the manner of lds_layout_dump.hip): the quad kernel's rule for taking reset
// positions from the draws wave OB makes ahead (csrc/pw_kernels_spread_quad.hpp quad_draw_engages), tabulated, and its pieces of the
// draw itself held against include/pworld_math.h on the host.  Lines:
//     depth <kQuadDrawDepth> slices <kQuadDrawSlices> rounds <kQuadDrawRounds> delay <kQuadDrawDelay>
//     rule <auto_reset> <max_episode_len> <clocks_equal> <steps_since_start> <0|1>
//     at <i> <float2 index of entry i>
//     draws <number compared> <number that differ from pw_reset_xy in any bit>
// Build: hipcc --offload-host-only -std=c++17 -I csrc -I include.
#include <cstdio>
#include <cstring>

#include "pw_kernels_spread_quad.hpp"

int main()
{
    std::printf("depth %d slices %d rounds %d delay %d\n", kQuadDrawDepth, kQuadDrawSlices, kQuadDrawRounds, kQuadDrawDelay);
    for (int ar = 0; ar <= 1; ++ar)
        for (int len = 0; len <= 30; ++len)
            for (int eq = 0; eq <= 1; ++eq)
                for (int since = -2; since <= 30; ++since)
                    std::printf("rule %d %d %d %d %d\n", ar, len, eq, since, quad_draw_engages(ar, len, eq != 0, since) ? 1 : 0);
    for (int i = 0; i < kQuadEPW * kQuadN; ++i) std::printf("at %d %d\n", i, quad_draw_at(i));
    // the draw in slices, as wave OB runs it: state kept between the slices, the keys of a slice from its index
    int n = 0, bad = 0;
    const uint64_t seeds[] = {0u, 43u, 0x9E3779B97F4A7C15ull}, bases[] = {0u, 1000u, (1ull << 32) + 5u, ~0ull - 70u};
    for (uint64_t seed : seeds)
        for (uint64_t base : bases)
            for (uint64_t e = 0; e < 64; e += 9)
                for (uint32_t ep : {0u, 1u, 2u, 77u, 0xFFFFFFFFu})
                    for (uint32_t ent = 0; ent < 12; ++ent) {
                        const uint64_t env_id = base + e;
                        uint32_t c[4] = {ent, ep, (uint32_t)env_id, (uint32_t)(env_id >> 32)};
                        for (int ph = 0; ph < kQuadDrawSlices; ++ph) {
                            uint32_t k0 = (uint32_t)seed + (uint32_t)(ph * kQuadDrawRounds) * 0x9E3779B9u;
                            uint32_t k1 = (uint32_t)(seed >> 32) + (uint32_t)(ph * kQuadDrawRounds) * 0xBB67AE85u;
                            for (int r = 0; r < kQuadDrawRounds; ++r) {
                                quad_philox_round(c, k0, k1);
                                k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
                            }
                        }
                        const float2 d = quad_draw_xy(c[0], c[1]);
                        float x, y;
                        pw_reset_xy(seed, env_id, ep, ent, -1.0f, 1.0f, &x, &y);
                        ++n;
                        bad += std::memcmp(&d.x, &x, 4) != 0 || std::memcmp(&d.y, &y, 4) != 0;
                    }
    std::printf("draws %d %d\n", n, bad);
    return 0;
}
