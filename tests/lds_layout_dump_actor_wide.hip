// Host-only program of tests/test_actor_wide_host.py, in the style of tests/lds_layout_dump.hip: prints, for the LDS layout functions of
// the one-launch actor (actor_lds) and of the chain's front end (actor_front_lds), csrc/pw_kernels_policy.hpp, at the stage-1 step counts
// of observation rows of 65 .. 104 numbers (S1 = 4 * S1C, S1C = 9 .. 13), one line
//     actor_front S1=<s> | actor_fused S1=<s>\t<bytes>\t<name:align:alias,...>\t<offset size offset size ...>
// `size` and `align` are stated HERE, from what the kernel reads and writes in the region (align: 16 for float4 accesses, 4 otherwise);
// the offsets and the total are the layout function's.  Build: hipcc --offload-host-only -std=c++17 -I csrc -I include.
#include <cstdio>
#include <string>

#include "pw_kernels_policy.hpp"

namespace {

alignas(16) unsigned char g_lds[1 << 20];    // larger than any layout formed below

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

}  // namespace

int main()
{
    char key[64];
    for (int S1C = 9; S1C <= 13; ++S1C) {
        const int S1 = 4 * S1C;
        {
            const ActorFrontLds o = actor_front_lds(S1, g_lds);
            Line l;
            // the kernel fills f_wih and f_w1 with ONE float4 copy loop: f_w1 has to follow f_wih without a gap (the test checks it)
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
    }
    return 0;
}
