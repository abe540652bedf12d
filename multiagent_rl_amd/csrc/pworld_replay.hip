// libpworld.so, fifth translation unit -- the replay ring (pw_replay_add*, pw_replay_gather, pw_replay_sample), transition packing (pw_pack_transitions,
// pw_exchange) and the three wire formats (pw_chunk_wire_*, pw_state_wire_*, pw_ref_wire_*).  The kernels are csrc/pw_kernels_replay.hpp; of the
// environment only the handle is used (pw_state_wire_begin / _finalize).  Declared in include/pworld.h; the error text is shared with pworld.hip.
#include "pw_host.hpp"
#include "pw_handle.hpp"
#include "pw_kernels_replay.hpp"

namespace {

void fill_wire(int32_t T, int32_t B, int32_t N, int32_t D, int32_t F, pw_chunk_wire *out)
{
    std::memset(out, 0, sizeof(*out));
    out->T = T; out->B = B; out->N = N; out->D = D; out->F = F;
    const size_t row = (size_t)B * N * D * sizeof(float);
    PlaneAllocator plane;
    out->obs0 = plane(row);
    out->obs = plane((size_t)T * row);
    out->final_rows = plane((size_t)F * row);
    out->rew_shared = plane((size_t)T * B * sizeof(float));
    out->act = plane((size_t)T * B * N);
    out->fin_slot = plane((size_t)T * B);
    out->total_bytes = plane.off;
}

int check_wire(const pw_chunk_wire *w, const void *wire)
{
    if (!w || !wire) return fail(PW_EINVAL, "null argument");
    if (w->T < 1 || w->B < 1 || w->N < 1 || w->D < 1 || w->F < 0 || w->F > 254) return fail(PW_EINVAL, "bad wire layout");
    pw_chunk_wire ref;  // offsets are not trusted blindly: they must be the ones pw_chunk_wire_layout produces
    fill_wire(w->T, w->B, w->N, w->D, w->F, &ref);
    if (ref.obs0 != w->obs0 || ref.obs != w->obs || ref.final_rows != w->final_rows || ref.rew_shared != w->rew_shared ||
        ref.act != w->act || ref.fin_slot != w->fin_slot || ref.total_bytes != w->total_bytes)
        return fail(PW_EINVAL, "wire layout was not produced by pw_chunk_wire_layout");
    if (reinterpret_cast<uintptr_t>(wire) & 255) return fail(PW_EINVAL, "wire block must be 256-byte aligned");
    return PW_OK;
}

int state_wire_row_dim(int scenario, int N, int L, int A)
{
    if (scenario == PW_SIMPLE_SPREAD) return 4 + 2 * L;
    if (scenario == PW_SIMPLE_TAG) return 4 + 2 * L + 2 * (N - 1) + 2 * (N - A);
    return -1;
}

void fill_state_wire(int32_t scenario, int32_t T, int32_t B, int32_t N, int32_t L, int32_t A, int32_t F, pw_state_wire *out)
{
    std::memset(out, 0, sizeof(*out));
    out->T = T; out->B = B; out->N = N; out->L = L; out->D = state_wire_row_dim(scenario, N, L, A); out->F = F;
    out->scenario = scenario; out->num_adversaries = A;
    const size_t st = (size_t)B * N * sizeof(float4);
    PlaneAllocator plane;
    out->state0 = plane(st);
    out->state = plane((size_t)T * st);
    out->final_state = plane((size_t)F * st);
    out->lm = plane((size_t)(F + 1) * B * L * sizeof(float2));
    out->ep0 = plane((size_t)B * sizeof(uint32_t));
    out->rew_shared = plane((size_t)T * B * sizeof(float));
    out->act = plane((size_t)T * B * N);
    out->epi = plane((size_t)T * B);
    out->total_bytes = plane.off;
}

int check_state_wire(const pw_state_wire *w, const void *wire)
{
    if (!w || !wire) return fail(PW_EINVAL, "null argument");
    if (w->T < 1 || w->B < 1 || w->N < 1 || w->L < 0 || w->F < 0 || w->F > 126 || w->num_adversaries < 0 || w->num_adversaries > w->N ||
        w->D < 4 || w->D != state_wire_row_dim(w->scenario, w->N, w->L, w->num_adversaries))
        return fail(PW_EINVAL, "bad state-wire layout");
    pw_state_wire ref;  // offsets must be the ones pw_state_wire_layout produces
    fill_state_wire(w->scenario, w->T, w->B, w->N, w->L, w->num_adversaries, w->F, &ref);
    if (std::memcmp(&ref, w, sizeof(ref)) != 0) return fail(PW_EINVAL, "wire layout was not produced by pw_state_wire_layout");
    if (reinterpret_cast<uintptr_t>(wire) & 255) return fail(PW_EINVAL, "wire block must be 256-byte aligned");
    return PW_OK;
}

int state_wire_handle_ok(const pw_handle *h, const pw_state_wire *w)
{
    if (!h) return fail(PW_EINVAL, "null handle");
    const bool spread = h->cfg.scenario == PW_SIMPLE_SPREAD && h->cfg.obs_mode == PW_OBS_LOCAL;
    const bool tag = h->cfg.scenario == PW_SIMPLE_TAG;
    if (!(spread || tag) || h->kp.D != state_wire_row_dim(h->cfg.scenario, h->kp.N, h->kp.L, h->kp.A))
        return fail(PW_EINVAL, "state-only wire blocks serve simple_spread with the local observation and simple_tag (rows that are a "
                               "function of {vel, pos} and the landmarks); use pw_chunk_wire_* elsewhere");
    if (w && (w->scenario != h->cfg.scenario || w->B != h->kp.B || w->N != h->kp.N || w->L != h->kp.L ||
              (tag && w->num_adversaries != h->kp.A)))
        return fail(PW_EINVAL, "wire / handle shape mismatch");
    return PW_OK;
}

void fill_ref_wire(int32_t T, int32_t B, int32_t F, pw_ref_wire *out)
{
    std::memset(out, 0, sizeof(*out));
    out->T = T; out->B = B; out->F = F;
    const size_t hd = (size_t)B * kRefN * kRefHead * sizeof(float);
    PlaneAllocator plane;
    out->head0 = plane(hd);
    out->head = plane((size_t)T * hd);
    out->final_head = plane((size_t)F * hd);
    out->goal = plane((size_t)(F + 1) * B * kRefN);
    out->comm0 = plane((size_t)B * kRefN);
    out->rew_shared = plane((size_t)T * B * sizeof(float));
    out->act = plane((size_t)T * B * kRefN * 2);
    out->epi = plane((size_t)T * B);
    out->total_bytes = plane.off;
}

int check_ref_wire(const pw_ref_wire *w, const void *wire)
{
    if (!w || !wire) return fail(PW_EINVAL, "null argument");
    if (w->T < 1 || w->B < 1 || w->F < 0 || w->F > 126) return fail(PW_EINVAL, "bad ref-wire layout");
    pw_ref_wire ref;
    fill_ref_wire(w->T, w->B, w->F, &ref);
    if (std::memcmp(&ref, w, sizeof(ref)) != 0) return fail(PW_EINVAL, "wire layout was not produced by pw_ref_wire_layout");
    if (reinterpret_cast<uintptr_t>(wire) & 255) return fail(PW_EINVAL, "wire block must be 256-byte aligned");
    return PW_OK;
}

// The *_agents wire entry points (0.1.23) write per-agent rings only and read the reward from the trailer plane rew_agents [T,B,N].
int agents_ring_only(const pw_replay_store *st, const float *rew_agents, const char *who, const char *plain)
{
    if (!st->per_agent)
        return fail(PW_EINVAL, std::string(who) + ": a shared-reward ring (per_agent = 0) is filled by " + plain + " (this entry point writes rew / done [cap,N])");
    if (!rew_agents || (reinterpret_cast<uintptr_t>(rew_agents) & 3))
        return fail(PW_EINVAL, std::string(who) + ": rew_agents must be a 4-byte aligned device pointer to the per-agent reward plane [T,B,N]");
    return PW_OK;
}

// Every refusal of an *_agents entry point names it (the checks it shares with the plain entry point do not know who asked).
int named(const char *who, int rc)
{
    if (rc == PW_OK) return rc;
    const std::string msg = pw_last_error();
    return msg.find(who) == std::string::npos ? fail(rc, std::string(who) + ": " + msg) : rc;
}

}  // namespace

extern "C" {

int pw_counter_add(int64_t *counter, int64_t delta, int64_t modulo, void *stream)
{
    if (!counter) return fail(PW_EINVAL, "null counter");
    hipLaunchKernelGGL(pw_counter_add_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), counter, delta, modulo);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

int pw_replay_add(const pw_replay_store *st, int64_t start, const int64_t *start_dev, int32_t B, const float *obs,
                  const int32_t *act_idx, const float *rew_shared, const float *next_obs, const float *final_obs,
                  const uint8_t *terminal, const float *done, void *stream)
{
    if (!st || !obs || !act_idx || !rew_shared || !next_obs) return fail(PW_EINVAL, "null argument");
    if (st->state_rows) return fail(PW_EINVAL, "pw_replay_add: a STATE ring is filled by pw_replay_add_state_wire only (rows do not determine the landmarks)");
    if (B < 1 || !ring_fits(st, B, start)) return fail(PW_EINVAL, "bad ring arguments");
    if (st->obs_dim < 2) return fail(PW_EINVAL, "obs_dim must be >= 2");
    if (st->act_heads < 0 || st->act_heads > 2 || (st->act_heads == 2 && (st->head_width[0] < 0 || st->head_width[1] < 1)))
        return fail(PW_EINVAL, "bad act_heads / head_width");
    const size_t total = (size_t)B * st->num_agents * st->obs_dim;
    hipLaunchKernelGGL(pw_replay_add_kernel, dim3(grid_blocks(total, 8192)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       *st, start, start_dev, B, obs, act_idx, rew_shared, next_obs, final_obs, terminal, done);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

int pw_replay_add_tail(const pw_replay_store *st, int64_t start, const int64_t *start_dev, int64_t *next_start_dev,
                       int32_t B, const float *obs, const int32_t *act_idx, const float *rew_shared,
                       const float *next_obs, const float *final_obs, const uint8_t *terminal, const float *done,
                       float *episode_return, double *finished_sum, int64_t *finished_count, int64_t *step_counter,
                       void *stream)
{
    if (!st || !obs || !act_idx || !rew_shared || !next_obs || !terminal || !episode_return || !finished_sum ||
        !finished_count)
        return fail(PW_EINVAL, "null argument");
    if (int rc = plain_ring_only(st, "pw_replay_add_tail")) return rc;
    if (B < 1 || !ring_fits(st, B, start)) return fail(PW_EINVAL, "bad ring arguments");
    if (st->obs_dim < 5) return fail(PW_EINVAL, "obs_dim must be >= 5");
    if (start_dev && next_start_dev == start_dev)
        return fail(PW_EINVAL, "next_start_dev must not alias start_dev (every workgroup reads start_dev)");
    const size_t total = (size_t)B * st->num_agents * st->obs_dim;
    const ReplayTail tl = {episode_return, finished_sum, finished_count, next_start_dev, step_counter};
    hipLaunchKernelGGL(pw_replay_add_tail_kernel, dim3(grid_blocks(total, 8192) + 1), dim3(256), 0, static_cast<hipStream_t>(stream),
                       *st, start, start_dev, B, obs, act_idx, rew_shared, next_obs, final_obs, terminal, done, tl);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

int pw_replay_add_rollout(const pw_replay_store *st, int64_t start, int32_t B, int32_t T, const float *obs0,
                          const pw_step_io *io, const int32_t *act, float *episode_return, double *finished_sum,
                          int64_t *finished_count, void *scratch, void *stream)
{
    if (!st || !obs0 || !io || !act || !io->obs || !io->rew_shared || !io->terminal) return fail(PW_EINVAL, "null argument");
    if (st->per_agent && !io->rew) return fail(PW_EINVAL, "pw_replay_add_rollout: a per-agent ring needs the chunk's per-agent rew [T,B,N]");
    if (st->state_rows) return fail(PW_EINVAL, "pw_replay_add_rollout: a STATE ring is filled by pw_replay_add_state_wire only");
    if (B < 1 || T < 1 || !ring_fits(st, (int64_t)B * T, start))
        return fail(PW_EINVAL, "bad ring arguments (the chunk must fit the ring)");
    if (st->obs_dim < 5) return fail(PW_EINVAL, "obs_dim must be >= 5");
    // as pw_replay_add / pw_replay_gather: the kernel stores one index per agent unless act_heads == 2, the gather reads two for any act_heads > 1
    if (st->act_heads < 0 || st->act_heads > 2 || (st->act_heads == 2 && (st->head_width[0] < 0 || st->head_width[1] < 1)))
        return fail(PW_EINVAL, "bad act_heads / head_width");
    if (st->act_heads == 2 && st->num_agents * st->obs_dim < 2 * st->num_agents) return fail(PW_EINVAL, "two-head ring: rows too short");
    if (episode_return && (!finished_sum || !finished_count || !scratch))
        return fail(PW_EINVAL, "bookkeeping needs episode_return, finished_sum, finished_count and scratch");
    const size_t total = (size_t)T * B * st->num_agents * st->obs_dim;
    const unsigned stat_blocks = episode_return ? (unsigned)((B + 255) / 256) : 0;
    const ReplayTail tl = {episode_return, finished_sum, finished_count, nullptr, nullptr};
    hipLaunchKernelGGL(pw_replay_add_rollout_kernel, dim3(grid_blocks(total, 16384) + stat_blocks), dim3(256), 0,
                       static_cast<hipStream_t>(stream), *st, start, B, T, obs0, *io, act, tl, stat_blocks,
                       static_cast<unsigned long long *>(scratch));
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

size_t pw_replay_add_rollout_scratch_bytes(int32_t B) { return (size_t)(2 * ((B + 255) / 256) + 1) * 8; }

int pw_replay_gather(const pw_replay_store *st, const int64_t *idx, int32_t b, float *out_obs, float *out_act,
                     float *out_rew, float *out_next_obs, float *out_done, void *stream)
{
    if (!st || !idx) return fail(PW_EINVAL, "null argument");
    if (b < 1) return fail(PW_EINVAL, "batch must be >= 1");
    if (st->obs_dim < 2) return fail(PW_EINVAL, "obs_dim must be >= 2");
    if (st->act_heads < 0 || st->act_heads > 2 || (st->act_heads == 2 && (st->head_width[0] < 0 || st->head_width[1] < 1)))
        return fail(PW_EINVAL, "bad act_heads / head_width");
    if (st->state_rows) {  // STATE ring: the rows are rebuilt from the slot's states and landmarks
        if (int rc = state_ring_ok(st, "pw_replay_gather")) return rc;
        if ((reinterpret_cast<uintptr_t>(out_obs) | reinterpret_cast<uintptr_t>(out_next_obs)) & 7)
            return fail(PW_EINVAL, "pw_replay_gather (STATE ring): out_obs / out_next_obs must be 8-byte aligned");
        const size_t units = (size_t)b * st->num_agents * (st->obs_dim / 2);
        hipLaunchKernelGGL(pw_replay_gather_state_kernel, dim3(grid_blocks(units, 8192)), dim3(256), 0, static_cast<hipStream_t>(stream),
                           *st, idx, b, out_obs, out_act, out_rew, out_next_obs, out_done);
        PW_HIP_CHECK(hipGetLastError());
        return PW_OK;
    }
    const size_t total = (size_t)b * st->num_agents * st->obs_dim;
    hipLaunchKernelGGL(pw_replay_gather_kernel, dim3(grid_blocks(total, 8192)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       *st, idx, b, out_obs, out_act, out_rew, out_next_obs, out_done);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

int64_t pw_replay_draw_host(uint64_t seed, int64_t call, int64_t e, int64_t len)
{
    return pw_replay_draw(seed, call, e, pw_replay_clamp_len(len, (int64_t)1 << 32));
}

int pw_replay_sample(const pw_replay_store *st, uint64_t seed, const int64_t *call_dev, const int64_t *len_dev, int32_t b,
                     int64_t *out_idx, float *out_obs, float *out_act, float *out_rew, float *out_next_obs, float *out_done,
                     void *stream)
{
    if (!st) return fail(PW_EINVAL, "pw_replay_sample: st is null");
    if (!call_dev) return fail(PW_EINVAL, "pw_replay_sample: call_dev is null (the device cell that numbers the draw)");
    if (!len_dev) return fail(PW_EINVAL, "pw_replay_sample: len_dev is null (the device cell that holds the ring's length)");
    if (b < 1) return fail(PW_EINVAL, "pw_replay_sample: b must be >= 1");
    const bool gather = out_obs || out_act || out_rew || out_next_obs || out_done;
    if (!out_idx && !gather)
        return fail(PW_EINVAL, "pw_replay_sample: out_idx, out_obs, out_act, out_rew, out_next_obs and out_done are all null (nothing to write)");
    if (st->capacity < 1 || st->capacity > ((int64_t)1 << 32))
        return fail(PW_EINVAL, "pw_replay_sample: st->capacity must be in [1, 2^32] (the draw scales one 32-bit word)");
    if ((reinterpret_cast<uintptr_t>(call_dev) | reinterpret_cast<uintptr_t>(len_dev) | reinterpret_cast<uintptr_t>(out_idx)) & 7)
        return fail(PW_EINVAL, "pw_replay_sample: call_dev, len_dev and out_idx must be 8-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!gather) {  // the draw alone: ReplayBuffer.make_index
        hipLaunchKernelGGL(pw_replay_draw_kernel, dim3(grid_blocks((size_t)b, 1024)), dim3(256), 0, s, *st, seed, call_dev, len_dev, b, out_idx);
        PW_HIP_CHECK(hipGetLastError());
        return PW_OK;
    }
    if (st->obs_dim < 2) return fail(PW_EINVAL, "pw_replay_sample: st->obs_dim must be >= 2");
    if (st->act_heads < 0 || st->act_heads > 2 || (st->act_heads == 2 && (st->head_width[0] < 0 || st->head_width[1] < 1)))
        return fail(PW_EINVAL, "pw_replay_sample: bad st->act_heads / st->head_width");
    if (st->state_rows) {  // STATE ring: the rows are rebuilt from the drawn slot's states and landmarks
        if (int rc = state_ring_ok(st, "pw_replay_sample")) return rc;
        if ((reinterpret_cast<uintptr_t>(out_obs) | reinterpret_cast<uintptr_t>(out_next_obs)) & 7)
            return fail(PW_EINVAL, "pw_replay_sample (STATE ring): out_obs / out_next_obs must be 8-byte aligned");
        const size_t units = (size_t)b * st->num_agents * (st->obs_dim / 2);
        hipLaunchKernelGGL(pw_replay_sample_state_kernel, dim3(grid_blocks(units, 8192)), dim3(256), 0, s, *st, seed, call_dev, len_dev, b,
                           out_idx, out_obs, out_act, out_rew, out_next_obs, out_done);
        PW_HIP_CHECK(hipGetLastError());
        return PW_OK;
    }
    const size_t total = (size_t)b * st->num_agents * st->obs_dim;
    hipLaunchKernelGGL(pw_replay_sample_kernel, dim3(grid_blocks(total, 8192)), dim3(256), 0, s, *st, seed, call_dev, len_dev, b, out_idx,
                       out_obs, out_act, out_rew, out_next_obs, out_done);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

int pw_pack_transitions(const pw_step_io *io, int32_t B, int32_t N, int32_t D, const int32_t *sel_t,
                        const int32_t *sel_e, int32_t R, float *rows, void *stream)
{
    if (!io || !sel_t || !sel_e || !rows) return fail(PW_EINVAL, "null argument");
    if (!io->obs || !io->act_idx || !io->rew_shared) return fail(PW_EINVAL, "chunk needs obs, act_idx and rew_shared");
    if (B < 1 || N < 1 || D < 1 || R < 1) return fail(PW_EINVAL, "bad sizes");
    const size_t total = (size_t)R * (2 * (size_t)N * D + N + 2);
    hipLaunchKernelGGL(pw_pack_transitions_kernel, dim3(grid_blocks(total, 4096)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       *io, B, N, D, sel_t, sel_e, R, rows);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

int pw_replay_add_packed(const pw_replay_store *st, int64_t start, int32_t R, const float *rows, void *stream)
{
    if (!st || !rows) return fail(PW_EINVAL, "null argument");
    if (int rc = plain_ring_only(st, "pw_replay_add_packed")) return rc;
    if (R < 1 || !ring_fits(st, R, start)) return fail(PW_EINVAL, "bad ring arguments");
    const size_t total = (size_t)R * (2 * (size_t)st->num_agents * st->obs_dim + st->num_agents + 2);
    hipLaunchKernelGGL(pw_replay_add_packed_kernel, dim3(grid_blocks(total, 4096)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       *st, start, R, rows);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

int pw_exchange(const pw_replay_store *st, int64_t start, int32_t R_in, const float *rows_in, const pw_step_io *io,
                int32_t B, int32_t N, int32_t D, const int32_t *sel_t, const int32_t *sel_e, int32_t R_out,
                float *rows_out, void *stream)
{
    const bool ingest = st && rows_in && R_in > 0;
    const bool pack = io && rows_out && R_out > 0;
    if (int rc = plain_ring_only(st, "pw_exchange")) return rc;
    if (!ingest && !pack) return fail(PW_EINVAL, "nothing to do");
    if (ingest && !ring_fits(st, R_in, start)) return fail(PW_EINVAL, "bad ring arguments");
    if (pack && (!sel_t || !sel_e || !io->obs || !io->act_idx || !io->rew_shared || B < 1 || N < 1 || D < 1))
        return fail(PW_EINVAL, "chunk needs obs, act_idx, rew_shared and a selection");
    if (ingest && pack && (st->num_agents != N || st->obs_dim != D)) return fail(PW_EINVAL, "row width mismatch");
    const int Nn = pack ? N : st->num_agents, Dd = pack ? D : st->obs_dim;
    const size_t W = 2 * (size_t)Nn * Dd + Nn + 2;
    const int nb_in = ingest ? (int)grid_blocks((size_t)R_in * W, 2048) : 0, nb_out = pack ? (int)grid_blocks((size_t)R_out * W, 2048) : 0;
    const pw_replay_store dummy_st = {};
    const pw_step_io dummy_io = {};
    hipLaunchKernelGGL(pw_exchange_kernel, dim3((unsigned)(nb_in + nb_out)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       ingest ? *st : dummy_st, start, ingest ? R_in : 0, rows_in, nb_in, pack ? *io : dummy_io, B, Nn, Dd,
                       sel_t, sel_e, pack ? R_out : 0, rows_out);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

int pw_chunk_wire_layout(int32_t T, int32_t B, int32_t N, int32_t D, int32_t max_episode_len, pw_chunk_wire *out)
{
    if (!out) return fail(PW_EINVAL, "null argument");
    if (T < 1 || B < 1 || N < 1 || D < 1 || max_episode_len < 0) return fail(PW_EINVAL, "bad sizes");
    int32_t F;
    if (int rc = episode_ends_per_chunk(T, max_episode_len, 254, &F)) return rc;
    fill_wire(T, B, N, D, F, out);
    return PW_OK;
}

int pw_chunk_wire_finalize(const pw_chunk_wire *w, void *wire, const float *obs0, const float *final_obs,
                           const uint8_t *terminal, const int32_t *act, void *stream)
{
    if (int rc = check_wire(w, wire)) return rc;
    if (!obs0 || !terminal || !act) return fail(PW_EINVAL, "null argument");
    const unsigned row_blocks = (unsigned)(((size_t)w->B * w->N * w->D + 255) / 256);
    const unsigned act_blocks = grid_blocks((size_t)w->T * w->B * w->N, 2048);
    hipLaunchKernelGGL(pw_chunk_wire_finalize_kernel, dim3(row_blocks + act_blocks), dim3(256), 0,
                       static_cast<hipStream_t>(stream), *w, wire, obs0, final_obs, terminal, act, row_blocks);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

// pw_replay_add_wire (rew_agents == nullptr, who == nullptr) and pw_replay_add_wire_agents share every check but the ring's kind.
static int add_wire(const pw_replay_store *st, int64_t start, const pw_chunk_wire *w, const void *wire, const float *rew_agents, const char *who,
                    void *stream)
{
    if (!st) return fail(PW_EINVAL, "null argument");
    if (who) {
        if (int rc = agents_ring_only(st, rew_agents, who, "pw_replay_add_wire")) return rc;
        if (int rc = row_ring_only(st, who)) return rc;
    } else if (int rc = plain_ring_only(st, "pw_replay_add_wire")) {
        return rc;
    }
    if (int rc = check_wire(w, wire)) return rc;
    if (st->num_agents != w->N || st->obs_dim != w->D) return fail(PW_EINVAL, "ring / wire shape mismatch");
    if (!ring_fits(st, (int64_t)w->T * w->B, start))
        return fail(PW_EINVAL, "bad ring arguments (the chunk must fit the ring)");
    const int ND = w->N * w->D;
    const bool vec = ND % 4 == 0 && ((reinterpret_cast<uintptr_t>(st->obs) | reinterpret_cast<uintptr_t>(st->next_obs)) & 15) == 0;
    const dim3 grid(grid_blocks((size_t)w->T * w->B * (vec ? ND / 4 : ND), 16384));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (who)
        hipLaunchKernelGGL(vec ? pw_replay_add_wire_agents_kernel<4> : pw_replay_add_wire_agents_kernel<1>, grid, dim3(256), 0, s, *st, start, *w, wire,
                           rew_agents);
    else
        hipLaunchKernelGGL(vec ? pw_replay_add_wire_kernel<4> : pw_replay_add_wire_kernel<1>, grid, dim3(256), 0, s, *st, start, *w, wire);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

int pw_replay_add_wire(const pw_replay_store *st, int64_t start, const pw_chunk_wire *w, const void *wire, void *stream)
{
    return add_wire(st, start, w, wire, nullptr, nullptr, stream);
}

int pw_replay_add_wire_agents(const pw_replay_store *st, int64_t start, const pw_chunk_wire *w, const void *wire, const float *rew_agents,
                              void *stream)
{
    return named("pw_replay_add_wire_agents", add_wire(st, start, w, wire, rew_agents, "pw_replay_add_wire_agents", stream));
}

size_t pw_wire_agent_rew_bytes(int32_t T, int32_t B, int32_t N)
{
    if (T < 1 || B < 1 || N < 1) return 0;
    return align_up((size_t)T * B * N * sizeof(float), 256);
}

int pw_state_wire_layout_scn(int32_t scenario, int32_t T, int32_t B, int32_t N, int32_t L, int32_t num_adversaries,
                             int32_t max_episode_len, pw_state_wire *out)
{
    if (!out) return fail(PW_EINVAL, "null argument");
    if (scenario != PW_SIMPLE_SPREAD && scenario != PW_SIMPLE_TAG)
        return fail(PW_EINVAL, "state-only wire blocks serve simple_spread (local observation) and simple_tag");
    if (scenario == PW_SIMPLE_SPREAD) num_adversaries = 0;
    if (T < 1 || B < 1 || N < 1 || L < 0 || max_episode_len < 0 || num_adversaries < 0 || num_adversaries > N) return fail(PW_EINVAL, "bad sizes");
    int32_t F;
    if (int rc = episode_ends_per_chunk(T, max_episode_len, 126, &F)) return rc;
    fill_state_wire(scenario, T, B, N, L, num_adversaries, F, out);
    return PW_OK;
}

int pw_state_wire_layout(int32_t T, int32_t B, int32_t N, int32_t L, int32_t max_episode_len, pw_state_wire *out)
{
    return pw_state_wire_layout_scn(PW_SIMPLE_SPREAD, T, B, N, L, 0, max_episode_len, out);
}

int pw_state_wire_begin(const pw_handle *h, const pw_state_wire *w, void *wire, void *stream)
{
    if (int rc = check_ready(h)) return rc;
    if (int rc = check_state_wire(w, wire)) return rc;
    if (int rc = state_wire_handle_ok(h, w)) return rc;
    const KParams &kp = h->kp;
    const size_t n = (size_t)w->B * (w->N > w->L ? w->N : w->L);
    hipLaunchKernelGGL(pw_state_wire_begin_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       *w, wire, kp.pos_x, kp.pos_y, kp.vel_x, kp.vel_y, kp.lm_x, kp.lm_y, kp.ep_count);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

int pw_state_wire_finalize(const pw_handle *h, const pw_state_wire *w, void *wire, const float *obs, const float *final_obs,
                           const uint8_t *terminal, const int32_t *act, void *stream)
{
    if (int rc = check_state_wire(w, wire)) return rc;
    if (int rc = state_wire_handle_ok(h, w)) return rc;
    if (!obs || !terminal || !act) return fail(PW_EINVAL, "null argument");
    if ((reinterpret_cast<uintptr_t>(obs) | reinterpret_cast<uintptr_t>(final_obs)) & 7)
        return fail(PW_EINVAL, "obs and final_obs must be 8-byte aligned");
    const size_t BN = (size_t)w->B * w->N, total = (size_t)w->T * BN;
    const unsigned copy_blocks = grid_blocks(total, 8192);
    const unsigned env_blocks = (unsigned)((BN + 255) / 256);
    const unsigned act_blocks = grid_blocks(total, 2048);
    // the landmarks an in-chunk reset drew: simple_spread U(-1, 1), simple_tag U(-0.9, 0.9) (upstream reset_world)
    const float lm_lo = w->scenario == PW_SIMPLE_TAG ? -0.9f : -1.0f, lm_hi = w->scenario == PW_SIMPLE_TAG ? 0.9f : 1.0f;
    hipLaunchKernelGGL(pw_state_wire_finalize_kernel, dim3(copy_blocks + env_blocks + act_blocks), dim3(256), 0,
                       static_cast<hipStream_t>(stream), *w, wire, obs, final_obs, terminal, act, (uint64_t)h->kp.seed,
                       (uint64_t)h->kp.env_id_base, lm_lo, lm_hi, copy_blocks, env_blocks);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

static int add_state_wire(const pw_replay_store *st, int64_t start, const pw_state_wire *w, const void *wire, const float *rew_agents,
                          const char *who, void *stream)
{
    if (!st) return fail(PW_EINVAL, "null argument");
    if (who)
        if (int rc = agents_ring_only(st, rew_agents, who, "pw_replay_add_state_wire")) return rc;
    if (int rc = check_state_wire(w, wire)) return rc;
    if (st->num_agents != w->N || st->obs_dim != w->D) return fail(PW_EINVAL, "ring / wire shape mismatch");
    if (!ring_fits(st, (int64_t)w->T * w->B, start))
        return fail(PW_EINVAL, "bad ring arguments (the chunk must fit the ring)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t agents = (size_t)w->T * w->B * w->N;
    if (st->state_rows) {  // STATE ring: copy what the block carries; pw_replay_gather rebuilds the rows
        if (!who && st->per_agent)
            return fail(PW_EINVAL, "pw_replay_add_state_wire: a per-agent STATE ring is filled by the pw_policy_rollout sink only (the wire blocks carry the shared reward)");
        if (int rc = state_ring_ok(st, who ? who : "pw_replay_add_state_wire")) return rc;
        if (st->scenario != w->scenario || st->num_landmarks != w->L || st->num_adversaries != w->num_adversaries)
            return fail(PW_EINVAL, "STATE ring / wire scenario mismatch");
        const dim3 grid(grid_blocks(agents, 16384));
        if (who)
            hipLaunchKernelGGL(pw_replay_add_state_wire_to_state_ring_agents_kernel, grid, dim3(256), 0, s, *st, start, *w, wire, rew_agents);
        else
            hipLaunchKernelGGL(pw_replay_add_state_wire_to_state_ring_kernel, grid, dim3(256), 0, s, *st, start, *w, wire);
        PW_HIP_CHECK(hipGetLastError());
        return PW_OK;
    }
    if (int rc = who ? row_ring_only(st, who) : plain_ring_only(st, "pw_replay_add_state_wire")) return rc;
    const uintptr_t al = reinterpret_cast<uintptr_t>(st->obs) | reinterpret_cast<uintptr_t>(st->next_obs);
    if (al & 7) return fail(PW_EINVAL, "ring observation planes must be 8-byte aligned");
    if (w->scenario != PW_SIMPLE_SPREAD) {  // simple_tag: 8-byte units (other agents' states feed every row)
        const dim3 grid(grid_blocks(agents * (w->D / 2), 16384));
        if (who)
            hipLaunchKernelGGL(pw_replay_add_state_wire_units_agents_kernel, grid, dim3(256), 0, s, *st, start, *w, wire, rew_agents);
        else
            hipLaunchKernelGGL(pw_replay_add_state_wire_units_kernel, grid, dim3(256), 0, s, *st, start, *w, wire);
        PW_HIP_CHECK(hipGetLastError());
        return PW_OK;
    }
    const bool v4 = w->L % 2 == 0 && (al & 15) == 0;
    const dim3 grid(grid_blocks(agents * (v4 ? w->D / 4 : w->D / 2), 16384));
    if (who)
        hipLaunchKernelGGL(v4 ? pw_replay_add_state_wire_agents_kernel<4> : pw_replay_add_state_wire_agents_kernel<2>, grid, dim3(256), 0, s, *st, start,
                           *w, wire, rew_agents);
    else
        hipLaunchKernelGGL(v4 ? pw_replay_add_state_wire_kernel<4> : pw_replay_add_state_wire_kernel<2>, grid, dim3(256), 0, s, *st, start, *w, wire);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

int pw_replay_add_state_wire(const pw_replay_store *st, int64_t start, const pw_state_wire *w, const void *wire, void *stream)
{
    return add_state_wire(st, start, w, wire, nullptr, nullptr, stream);
}

int pw_replay_add_state_wire_agents(const pw_replay_store *st, int64_t start, const pw_state_wire *w, const void *wire, const float *rew_agents,
                                    void *stream)
{
    return named("pw_replay_add_state_wire_agents", add_state_wire(st, start, w, wire, rew_agents, "pw_replay_add_state_wire_agents", stream));
}

int pw_ref_wire_layout(int32_t T, int32_t B, int32_t max_episode_len, pw_ref_wire *out)
{
    if (!out) return fail(PW_EINVAL, "null argument");
    if (T < 1 || B < 1 || max_episode_len < 0) return fail(PW_EINVAL, "bad sizes");
    int32_t F;
    if (int rc = episode_ends_per_chunk(T, max_episode_len, 126, &F)) return rc;
    fill_ref_wire(T, B, F, out);
    return PW_OK;
}

int pw_ref_wire_finalize(const pw_ref_wire *w, void *wire, const float *obs0, const float *obs, const float *final_obs,
                         const uint8_t *terminal, const int32_t *act, void *stream)
{
    if (int rc = check_ref_wire(w, wire)) return rc;
    if (!obs0 || !obs || !terminal || !act) return fail(PW_EINVAL, "null argument");
    if (w->F > 0 && !final_obs) return fail(PW_EINVAL, "final_obs is needed when episodes end inside the chunk");
    const size_t BN = (size_t)w->B * kRefN;
    const unsigned copy_blocks = grid_blocks((size_t)w->T * BN * kRefHead, 8192);
    const unsigned env_blocks = (unsigned)((BN + 255) / 256);
    const unsigned act_blocks = grid_blocks((size_t)w->T * BN * 2, 2048);
    hipLaunchKernelGGL(pw_ref_wire_finalize_kernel, dim3(copy_blocks + env_blocks + act_blocks), dim3(256), 0,
                       static_cast<hipStream_t>(stream), *w, wire, obs0, obs, final_obs, terminal, act, copy_blocks, env_blocks);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

static int add_ref_wire(const pw_replay_store *st, int64_t start, const pw_ref_wire *w, const void *wire, const float *rew_agents, const char *who,
                        void *stream)
{
    if (!st) return fail(PW_EINVAL, "null argument");
    if (who)
        if (int rc = agents_ring_only(st, rew_agents, who, "pw_replay_add_ref_wire")) return rc;
    if (int rc = check_ref_wire(w, wire)) return rc;
    if (!who && st->per_agent)
        return fail(PW_EINVAL, "pw_replay_add_ref_wire: a per-agent ring is not served (the compact-row blocks carry the shared reward only)");
    if (st->state_rows || st->act_heads != 2 || st->head_width[1] != PW_DIM_C || (st->head_width[0] != 0 && st->head_width[0] != 5))
        return fail(PW_EINVAL, std::string(who ? who : "pw_replay_add_ref_wire") + ": the ring must be the two-head ring of simple_reference (act_heads = 2, head widths 5 | dim_c)");
    if (st->num_agents != kRefN || st->obs_dim != kRefD) return fail(PW_EINVAL, "ring / wire shape mismatch (simple_reference: N = 2, D = 21)");
    if (!ring_fits(st, (int64_t)w->T * w->B, start))
        return fail(PW_EINVAL, "bad ring arguments (the chunk must fit the ring)");
    const dim3 grid(grid_blocks((size_t)w->T * w->B * kRefN * kRefD, 16384));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (who)
        hipLaunchKernelGGL(pw_replay_add_ref_wire_agents_kernel, grid, dim3(256), 0, s, *st, start, *w, wire, rew_agents);
    else
        hipLaunchKernelGGL(pw_replay_add_ref_wire_kernel, grid, dim3(256), 0, s, *st, start, *w, wire);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

int pw_replay_add_ref_wire(const pw_replay_store *st, int64_t start, const pw_ref_wire *w, const void *wire, void *stream)
{
    return add_ref_wire(st, start, w, wire, nullptr, nullptr, stream);
}

int pw_replay_add_ref_wire_agents(const pw_replay_store *st, int64_t start, const pw_ref_wire *w, const void *wire, const float *rew_agents,
                                  void *stream)
{
    return named("pw_replay_add_ref_wire_agents", add_ref_wire(st, start, w, wire, rew_agents, "pw_replay_add_ref_wire_agents", stream));
}

}  // extern "C"
