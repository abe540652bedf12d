// Host-only program of tests/test_lstm_host.py, in the style of tests/lds_layout_dump_critic_steps.hip: prints, for the LDS layout function of
// the LSTM recurrence kernels (lstm_train_lds, csrc/pw_kernels_lstm.hpp) at both served shapes, forward and backward, one line
//     lstm_train H=<h> dirs=<d> backward=<0|1>\t<bytes>\t<name:align:alias,...>\t<offset size offset size ...>
// `size` and `align` are stated HERE, from what the kernels read and write in the region (16: float4 accesses); the offsets and the
// total are the layout function's.  Build: hipcc --offload-host-only -std=c++17 -I csrc -I include.
#include <cstdio>
#include <string>

#include "pw_kernels_lstm.hpp"

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
    const int shapes[2][2] = {{64, 1}, {32, 2}};
    for (const auto &s : shapes)
        for (int backward = 0; backward < 2; ++backward) {
            const int H = s[0], dirs = s[1], groups = 256 / H;
            const LstmTrainLds o = lstm_train_lds(H, dirs, backward != 0, g_lds);
            Line l;
            // W_hh of every direction, 4 H x H floats each, read as float4; one slot per (sequence, direction) of the workgroup for the vector
            // its lanes share, read as float4: h [H] forward, dG_t [4 H] backward
            l.r("w", o.s_w, (size_t)dirs * 4 * H * H * 4, 16); l.r("x", o.s_x, (size_t)groups * (backward ? 4 * H : H) * 4, 16);
            std::snprintf(key, sizeof key, "lstm_train H=%d dirs=%d backward=%d", H, dirs, backward);
            l.print(key, o.bytes);
        }
    return 0;
}
