// Host-only program of tests/test_policy_generic_host.py, in the style of tests/lds_layout_dump.hip: prints, for the LDS layout function
// of the generic one-launch policy rollout (policy_generic_lds, csrc/pw_kernels_policy_generic.hpp) and every shape with rows of at
// most 64 numbers and E * N <= 96 rows -- whether its launch size fits or not; the test knows which ones the host admits -- one line
//     policy_generic scen=<s> obs=<o> N=<n> L=<l> A=<a> E=<e>\t<bytes>\t<name:align:alias,...>\t<offset size offset size ...>
// `size` and `align` are stated HERE, from what the kernel reads and writes in the region (align: 16 for float4 accesses, 8 for float2 /
// double, 4 otherwise); the offsets and the total are the layout function's.  Build: hipcc --offload-host-only -std=c++17 -I csrc -I include.
#include <cstdio>
#include <string>

#include "pw_kernels_policy_generic.hpp"

namespace {

alignas(16) unsigned char g_lds[4 << 20];    // larger than any layout the loops below form

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

void shape(int scen, int obs, int N, int L, int A, int D)
{
    char key[128];
    const int S1 = 4 * ((D + 7) / 8);
    for (int E = 1; E <= 16 && E * N <= kFusedRows; ++E) {
        const PolicyGenericLds o = policy_generic_lds(S1, D, E, N, L, g_lds);
        const int rows = E * N, epw = E < kWave / N ? E : kWave / N, waves = (E + epw - 1) / epw;
        Line l;
        l.r("xf", o.a16.s_xf, (size_t)N * 4096, 16);
        l.r("hx", o.a16.s_hx, 8192, 16);
        l.r("hf", o.a16.s_hf, (size_t)((rows + 15) / 16) * 4096, 16);
        l.r("f_w1", o.a16.f_w1, (size_t)2 * S1 * 64 * 4, 16);
        l.r("b1", o.a16.s_b1, 256, 4);
        l.r("obs", o.s_obs, (size_t)rows * D * 4, 16); l.r("act", o.s_act, (size_t)rows * 4, 4);
        l.r("pos", o.s_pos, (size_t)waves * 512, 8); l.r("vel", o.s_vel, (size_t)waves * 512, 8);
        l.r("lm", o.s_lm, (size_t)waves * epw * L * 8, 8); l.r("redl", o.s_red, (size_t)waves * epw * L * 4, 4);
        l.r("fs", o.s_fs, 128, 8); l.r("fc", o.s_fc, 64, 4); l.r("noise", o.s_noise, (size_t)rows * 2 * 16, 16);
        l.r("red", o.red, 8192, 8, true);
        std::snprintf(key, sizeof key, "policy_generic scen=%d obs=%d N=%d L=%d A=%d E=%d", scen, obs, N, L, A, E);
        l.print(key, o.bytes);
    }
}

}  // namespace

int main()
{
    for (int N = 1; N <= PW_MAX_AGENTS; ++N)
        for (int L = 0; L <= PW_MAX_LANDMARKS; ++L) {
            const int dl = 4 + 2 * L, df = 4 + 2 * L + 4 * (N - 1);
            if (dl <= 64) shape(PW_SIMPLE_SPREAD, PW_OBS_LOCAL, N, L, 0, dl);
            if (df <= 64) shape(PW_SIMPLE_SPREAD, PW_OBS_FULL, N, L, 0, df);
            for (int A = 0; A <= N; ++A) {
                const int dt = 4 + 2 * L + 2 * (N - 1) + 2 * (A > 0 ? N - A : N - A - 1);
                if (dt >= 1 && dt <= 64) shape(PW_SIMPLE_TAG, PW_OBS_LOCAL, N, L, A, dt);
            }
        }
    return 0;
}
