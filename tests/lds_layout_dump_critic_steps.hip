// Host-only program of tests/test_bicnet_host.py, in the style of tests/lds_layout_dump_actor_wide.hip: prints, for the LDS layout function of
// the per-step critic (critic_steps_lds, csrc/pw_kernels_critic.hpp) at R = 16 and N = 1 .. 64, one line
//     critic_steps N=<n> R=16\t<bytes>\t<name:align:alias,...>\t<offset size offset size ...>
// `size` and `align` are stated HERE, from what the kernel reads and writes in the region (align: 16 for float4 accesses, 4 otherwise);
// the offsets and the total are the layout function's.  Build: hipcc --offload-host-only -std=c++17 -I csrc -I include.
#include <cstdio>
#include <string>

#include "pw_kernels_critic.hpp"

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
    const int R = 16, FR = 4 * R;
    for (int N = 1; N <= PW_MAX_AGENTS; ++N) {
        const CriticStepsLds o = critic_steps_lds(N, R, g_lds);
        Line l;
        // two slots of step outputs and four x1 buffers, each [4 fragments][FR] float4; the q staging [R][N] floats
        l.r("out", o.s_out, (size_t)2 * 4 * FR * 16, 16); l.r("x", o.s_x, (size_t)4 * 4 * FR * 16, 16); l.r("q", o.s_q, (size_t)R * N * 4, 4);
        std::snprintf(key, sizeof key, "critic_steps N=%d R=%d", N, R);
        l.print(key, o.bytes);
    }
    return 0;
}
