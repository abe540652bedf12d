// pw_replay_draw.hpp -- the batch draw of pw_replay_sample as one host / device function (csrc/pworld_replay.hip exports it to the
// host as pw_replay_draw_host, so the rule is testable without a GPU).
//
// The draw is stateless per element: element e of draw number `call` on a ring holding `len` transitions is
//   w   = word (e & 3) of Philox4x32-10(counter = (e >> 2, call lo, call hi, kReplayDrawTag), key = (seed lo, seed hi))
//   idx = ((u64)w * (u64)len) >> 32                    -- in [0, len) for every w, whatever len in [1, 2^32]
// Bias: the 2^32 words fall into len bins of floor(2^32 / len) or ceil(2^32 / len) words each, so a slot's probability is off
// by at most len / 2^32 relative (2.3e-4 at the 10^6-transition ring) -- the same kind of bias as the modulo in torch.randint.
//
// Philox streams of the library, all keyed (seed lo, seed hi); a counter is the four words (c0, c1, c2, c3):
//   reset draws   (pw_reset_xy, pworld_math.h)         (entity, episode, env_id lo, env_id hi)
//   Gumbel noise  (pw_gumbel_noise4, actor kernels)    (row lo, row hi | block tag in the two top bits, step lo, step hi)
//   batch draws   (here)                               (e >> 2, call lo, call hi, kReplayDrawTag)
// The batch draws meet the other two only where c3 == kReplayDrawTag, i.e. at an env id or a Philox step of at least
// 0x52504C59 * 2^32 (5.9e18): neither counter gets there (env ids count environments, steps count launches).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "pworld_math.h"

constexpr uint32_t kReplayDrawTag = 0x52504C59u;   // "RPLY"

// What a length cell may hold -> what the draw uses: an out-of-range slot is impossible whatever the cell says.
PW_HD int64_t pw_replay_clamp_len(int64_t len, int64_t capacity)
{
    if (len > capacity) len = capacity;
    return len < 1 ? 1 : len;
}

PW_HD int64_t pw_replay_draw(uint64_t seed, int64_t call, int64_t e, int64_t len)
{
    uint32_t w[4];
    pw_philox4x32_10((uint32_t)((uint64_t)e >> 2), (uint32_t)(uint64_t)call, (uint32_t)((uint64_t)call >> 32), kReplayDrawTag,
                     (uint32_t)seed, (uint32_t)(seed >> 32), w);
    const unsigned k = (unsigned)e & 3u;   // selects, not an indexed load: the four words stay in registers
    const uint32_t word = k == 0 ? w[0] : k == 1 ? w[1] : k == 2 ? w[2] : w[3];
    return (int64_t)(((uint64_t)word * (uint64_t)len) >> 32);
}
