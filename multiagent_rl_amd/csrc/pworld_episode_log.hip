// libpworld.so, fourteenth translation unit -- the episode log: pw_episode_log_absorb turns one chunk's rew [T,B,N] / terminal [T,B] planes
// into one log entry per finished episode (per-agent and total returns in float64, end step, env), in (end step, env) order, with the
// log's length, step count and running returns in device memory.  The kernels, their mapping and the summation order are
// csrc/pw_kernels_episode_log.hpp.  Declared in include/pworld.h; the error text is shared with pworld.hip.
#include "pw_host.hpp"
#include "pw_kernels_episode_log.hpp"

namespace {

// scratch: the header | tile_count [tiles] int32 | slot [T B] int32, each on a 256-byte boundary
struct EpisodeLogScratch {
    size_t tiles, tile_count, slot, bytes;
};

bool episode_log_scratch(int32_t T, int32_t B, EpisodeLogScratch *s)
{
    if (T < 1 || B < 1 || (int64_t)T * B > 0x7fffffff) return false;
    const size_t flags = (size_t)T * (size_t)B;
    PlaneAllocator at;
    at(sizeof(EpisodeLogHeader));
    s->tiles = (flags + kLogTile - 1) / kLogTile;
    s->tile_count = at(s->tiles * sizeof(int));
    s->slot = at(flags * sizeof(int));
    s->bytes = at.off;
    return true;
}

}  // namespace

extern "C" {

size_t pw_episode_log_scratch_bytes(int32_t T, int32_t B)
{
    EpisodeLogScratch s;
    return episode_log_scratch(T, B, &s) ? s.bytes : 0;
}

int pw_episode_log_absorb(const pw_episode_log *log, const float *rew, const uint8_t *terminal, int32_t T, void *stream)
{
    if (!log) return fail(PW_EINVAL, "log is null");
    if (log->struct_size != sizeof(pw_episode_log)) return fail(PW_EINVAL, "pw_episode_log.struct_size mismatch");
    const int32_t B = log->num_envs, N = log->num_agents;
    if (T < 1) return fail(PW_EINVAL, "T must be >= 1");
    if (B < 1) return fail(PW_EINVAL, "num_envs must be >= 1");
    if (N < 1 || N > PW_EPISODE_LOG_MAX_AGENTS) return fail(PW_EINVAL, "num_agents must be in 1 .. 96");
    if (log->capacity < 1) return fail(PW_EINVAL, "capacity must be >= 1");
    EpisodeLogScratch lay;
    if (!episode_log_scratch(T, B, &lay)) return fail(PW_EINVAL, "T * num_envs: more flags than the int32 slot plane holds (2^31 - 1)");
    if ((int64_t)B * (N + 1) >= ((int64_t)1 << 32))
        return fail(PW_EINVAL, "num_envs * (num_agents + 1): more walk threads than one launch's grid holds (2^32)");
    if (!rew) return fail(PW_EINVAL, "rew is null");
    if (!terminal) return fail(PW_EINVAL, "terminal is null");
    if (!log->total) return fail(PW_EINVAL, "total is null");
    if (!log->by_agent) return fail(PW_EINVAL, "by_agent is null");
    if (!log->end_step) return fail(PW_EINVAL, "end_step is null");
    if (!log->env) return fail(PW_EINVAL, "env is null");
    if (!log->carry) return fail(PW_EINVAL, "carry is null");
    if (!log->length) return fail(PW_EINVAL, "length is null");
    if (!log->step_base) return fail(PW_EINVAL, "step_base is null");
    if (!log->scratch) return fail(PW_EINVAL, "scratch is null");
    if (misaligned(rew)) return fail(PW_EINVAL, "rew must be 4-byte aligned");
    if (misaligned(log->total, 8)) return fail(PW_EINVAL, "total must be 8-byte aligned");
    if (misaligned(log->by_agent, 8)) return fail(PW_EINVAL, "by_agent must be 8-byte aligned");
    if (misaligned(log->end_step, 8)) return fail(PW_EINVAL, "end_step must be 8-byte aligned");
    if (misaligned(log->env)) return fail(PW_EINVAL, "env must be 4-byte aligned");
    if (misaligned(log->carry, 8)) return fail(PW_EINVAL, "carry must be 8-byte aligned");
    if (misaligned(log->length, 8)) return fail(PW_EINVAL, "length must be 8-byte aligned");
    if (misaligned(log->step_base, 8)) return fail(PW_EINVAL, "step_base must be 8-byte aligned");
    if (misaligned(log->scratch, 16)) return fail(PW_EINVAL, "scratch must be 16-byte aligned");

    char *base = static_cast<char *>(log->scratch);
    EpisodeLogHeader *header = reinterpret_cast<EpisodeLogHeader *>(base);
    int *tile_count = reinterpret_cast<int *>(base + lay.tile_count);
    int *slot = reinterpret_cast<int *>(base + lay.slot);
    const long long flags = (long long)T * B;
    const dim3 block(kLogThreads), tiles((unsigned)lay.tiles);
    const dim3 walkers((unsigned)(((long long)B * (N + 1) + kLogThreads - 1) / kLogThreads));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // checked after every launch: one that is refused leaves the rest unlaunched.  The cells advance in the second kernel, so a PW_EHIP
    // from the third or fourth leaves a log whose length counts entries that were never stored: the caller discards it.
    hipLaunchKernelGGL(pw_episode_log_count_kernel, tiles, block, 0, s, terminal, flags, tile_count);
    PW_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(pw_episode_log_offsets_kernel, dim3(1), block, 0, s, tile_count, (int)lay.tiles, (int)T,
                       reinterpret_cast<long long *>(log->length), reinterpret_cast<long long *>(log->step_base), header);
    PW_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(pw_episode_log_slots_kernel, tiles, block, 0, s, terminal, flags, tile_count, slot);
    PW_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(pw_episode_log_walk_kernel, walkers, block, 0, s, rew, terminal, slot, header, (int)T, (int)B, (int)N,
                       (long long)log->capacity, log->total, log->by_agent, reinterpret_cast<long long *>(log->end_step), log->env,
                       log->carry);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

}  // extern "C"
