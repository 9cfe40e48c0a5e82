// seeding.hip -- the seeding path (include/sdm_seeding.h): PySDM's `Seeding` dynamic
//
// Reference: PySDM/backends/impl_numba/methods/seeding_methods.py (one serial loop over all
// slots), PySDM/particulator.py:447-499, PySDM/dynamics/seeding.py.
//
// "The first K slots with multiplicity 0, in slot order, receive seeds 0 .. K-1" is an ordered
// selection.  Three launches on the stream, no workgroup ever waits for another:
//   k_seed_count    a workgroup per tile of SEED_TILE slots counts its zeros: a ballot and a
//                   popcount per 64 slots, summed through LDS
//   k_seed_scan     one workgroup: exclusive scan of the tile counts (SEED_ROUND counts a round),
//                   the check of the K seed indices, and the verdict - the total of zeros is known
//                   here, before any store, so a shortfall stores nothing
//   k_seed_scatter  a workgroup per tile again; a tile whose offset is not below K (or any tile
//                   after a refusal) exits after one compare, the others rank their zeros (ballot,
//                   popcount of the lanes below) and copy the seed's columns in
// With K far below n_sd the cost is one streaming read of the multiplicity column.  Rows are
// copied as 8-byte integers, so NaN payloads and signed zeros arrive as they are.
#include "common.h"
#include "index.h"
#include "../../include/sdm_seeding.h"

#define SEED_CHUNKS 4
#define SEED_TILE (SDM_BLOCK * SEED_CHUNKS)  // 1024 slots: 16 runs of 64, one ballot each
#define SEED_RUNS (SEED_TILE / SDM_WAVE)
#define SEED_ROUND (SDM_BLOCK * 4)           // tile counts per round of the scan
#define SEED_WAVES (SDM_BLOCK / SDM_WAVE)

namespace {

// control words of a call (device): SDM_SEED_STATUS_* first, then the gate the later kernels read
#define SEED_GATE 3  // 1: store; 0: refused (status word 3 of the header's four)

// chunk c of a tile is its slots [c * SDM_BLOCK, (c + 1) * SDM_BLOCK): thread t holds slot
// c * SDM_BLOCK + t, so wave w's ballot of chunk c covers run c * SEED_WAVES + w, 64 consecutive slots
__device__ __forceinline__ void tile_ballots(const int64_t *__restrict__ multiplicity,
                                             int64_t base, int64_t n_sd,
                                             unsigned long long zeros[SEED_CHUNKS]) {
#pragma unroll
  for (int c = 0; c < SEED_CHUNKS; ++c) {
    const int64_t i = base + c * SDM_BLOCK + threadIdx.x;
    const bool free_slot = i < n_sd && multiplicity[i] == 0;
    zeros[c] = __ballot(free_slot);
  }
}

__global__ void __launch_bounds__(SDM_BLOCK)
k_seed_count(const int64_t *__restrict__ multiplicity, int64_t n_sd,
             int32_t *__restrict__ tile_count) {
  __shared__ int s_wave[SEED_WAVES];
  unsigned long long zeros[SEED_CHUNKS];
  tile_ballots(multiplicity, (int64_t)blockIdx.x * SEED_TILE, n_sd, zeros);
  int count = 0;
#pragma unroll
  for (int c = 0; c < SEED_CHUNKS; ++c) count += __popcll(zeros[c]);
  if (lane_id() == 0) s_wave[threadIdx.x / SDM_WAVE] = count;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
#pragma unroll
    for (int w = 0; w < SEED_WAVES; ++w) total += s_wave[w];
    tile_count[blockIdx.x] = total;
  }
}

// one workgroup.  tile_offset[t] = zeros in the tiles before t; ctl: the status words and the gate;
// fctl (fused step, else NULL): the control block of the compaction that follows - "compact now"
// over all n_sd slots if the injection goes ahead, "healthy: nothing to do" if it is refused
__global__ void __launch_bounds__(SDM_BLOCK)
k_seed_scan(const int32_t *__restrict__ tile_count, int32_t *__restrict__ tile_offset,
            int64_t n_tiles, const int64_t *__restrict__ seed_index, int64_t n_seeds, int64_t K,
            int64_t n_sd, int64_t *__restrict__ ctl, int64_t *__restrict__ fctl) {
  __shared__ int64_t s_wave[SEED_WAVES];
  __shared__ int64_t s_carry, s_bad;
  const int lane = lane_id(), wave = threadIdx.x / SDM_WAVE;
  if (threadIdx.x == 0) {
    s_carry = 0;
    s_bad = 0;
  }
  __syncthreads();
  for (int64_t first = 0; first < n_tiles; first += SEED_ROUND) {
    const int64_t at = first + (int64_t)threadIdx.x * 4;
    int v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = at + e < n_tiles ? tile_count[at + e] : 0;
    const int64_t mine = (int64_t)v[0] + v[1] + v[2] + v[3];
    int64_t incl = mine;  // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < SDM_WAVE; o <<= 1) {
      const int64_t t = __shfl_up((long long)incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (lane == SDM_WAVE - 1) s_wave[wave] = incl;
    __syncthreads();
    int64_t before = s_carry, round_total = 0;
#pragma unroll
    for (int w = 0; w < SEED_WAVES; ++w) {
      if (w < wave) before += s_wave[w];
      round_total += s_wave[w];
    }
    int64_t run = before + incl - mine;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      // (beyond INT32_MAX never: n_sd is below it)
      if (at + e < n_tiles) tile_offset[at + e] = (int32_t)run;
      run += v[e];
    }
    __syncthreads();
    if (threadIdx.x == 0) s_carry += round_total;
    __syncthreads();
  }
  int64_t bad = 0;
  for (int64_t j = threadIdx.x; j < K; j += SDM_BLOCK) {
    const int64_t s = seed_index[j];
    bad += (s < 0 || s >= n_seeds) ? 1 : 0;
  }
  bad = wave_sum_i64(bad);
  if (lane == 0 && bad)
    atomicAdd((unsigned long long *)&s_bad, (unsigned long long)bad);  // (LDS)
  __syncthreads();
  if (threadIdx.x == 0) {
    const int64_t total = s_carry;
    const bool go = total >= K && s_bad == 0;
    ctl[SDM_SEED_STATUS_FREE] = total;
    ctl[SDM_SEED_STATUS_INJECTED] = go ? K : 0;
    ctl[SDM_SEED_STATUS_BAD_SEED] = s_bad;
    ctl[SEED_GATE] = go ? 1 : 0;
    if (fctl) {
      fctl[0] = n_sd;        // valid
      fctl[1] = n_sd;        // working
      fctl[2] = 0;           // sorted
      fctl[3] = go ? 0 : 1;  // healthy != 0: the compaction kernel returns at once
      fctl[4] = fctl[5] = fctl[6] = fctl[7] = 0;
    }
  }
}

__global__ void __launch_bounds__(SDM_BLOCK)
k_seed_scatter(int64_t *__restrict__ idx, int64_t *__restrict__ multiplicity,
               uint64_t *__restrict__ attributes, int64_t n_attr, int64_t n_sd,
               const int64_t *__restrict__ seed_index,
               const int64_t *__restrict__ seed_multiplicity,
               const uint64_t *__restrict__ seed_attributes, int64_t n_seeds, int64_t K,
               const int32_t *__restrict__ tile_offset, const int64_t *__restrict__ ctl) {
  const int64_t offset = tile_offset[blockIdx.x];
  if (offset >= K || ctl[SEED_GATE] == 0) return;  // (uniform over the workgroup)
  __shared__ int s_run[SEED_RUNS];
  const int lane = lane_id(), wave = threadIdx.x / SDM_WAVE;
  const int64_t base = (int64_t)blockIdx.x * SEED_TILE;
  unsigned long long zeros[SEED_CHUNKS];
  tile_ballots(multiplicity, base, n_sd, zeros);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < SEED_CHUNKS; ++c) s_run[c * SEED_WAVES + wave] = __popcll(zeros[c]);
  }
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1;
#pragma unroll
  for (int c = 0; c < SEED_CHUNKS; ++c) {
    if (!((zeros[c] >> lane) & 1)) continue;
    const int run = c * SEED_WAVES + wave;
    int64_t rank = offset + __popcll(zeros[c] & below);
    for (int r = 0; r < run; ++r) rank += s_run[r];
    if (rank >= K) continue;
    const int64_t i = base + c * SDM_BLOCK + threadIdx.x;
    const int64_t s = seed_index[rank];  // within [0, n_seeds): k_seed_scan looked
    multiplicity[i] = seed_multiplicity[s];
    for (int64_t a = 0; a < n_attr; ++a) attributes[a * n_sd + i] = seed_attributes[a * n_seeds + s];
    if (idx) idx[i] = -1;
  }
}

// ParticleAttributes.reset_idx of the fused step; index.hip's k_identity unless the injection was
// refused (then idx stays as it is, as the header promises)
__global__ void __launch_bounds__(SDM_BLOCK)
k_seed_identity(int64_t *__restrict__ idx, int64_t n, const int64_t *__restrict__ ctl) {
  if (ctl[SEED_GATE] == 0) return;
  const int64_t i = (int64_t)blockIdx.x * SDM_BLOCK + threadIdx.x;
  if (i < n) idx[i] = i;
}

struct SeedScratch {
  int32_t *tile_count, *tile_offset;
  int64_t *ctl, *fctl, *cctl;
  double *u01;
};

size_t seed_scratch_bytes(int64_t n_sd, int64_t n_seeds) {
  const size_t n_tiles = grid_for(n_sd, SEED_TILE);
  return 2 * carve_size(sizeof(int32_t) * n_tiles) + 3 * carve_size(sizeof(int64_t) * 8) +
         carve_size(sizeof(double) * (size_t)n_seeds);
}

SeedScratch seed_carve(char *base, int64_t n_sd, int64_t n_seeds) {
  Carver cv(base);
  const size_t n_tiles = grid_for(n_sd, SEED_TILE);
  SeedScratch s;
  s.tile_count = cv.take<int32_t>(n_tiles);
  s.tile_offset = cv.take<int32_t>(n_tiles);
  s.ctl = cv.take<int64_t>(8);
  s.fctl = cv.take<int64_t>(8);
  s.cctl = cv.take<int64_t>(8);
  s.u01 = cv.take<double>((size_t)n_seeds);
  return s;
}

// count, scan, scatter on the stream; `ctl` receives the status words and the gate
int inject_async(sdm_ctx *ctx, const SeedScratch &s, int64_t *idx, int64_t *multiplicity,
                 double *attributes, int64_t n_attr, int64_t n_sd, const int64_t *seed_index,
                 const int64_t *seed_multiplicity, const double *seed_attributes,
                 int64_t n_seeds, int64_t K, int64_t *ctl, int64_t *fctl) {
  const unsigned n_tiles = grid_for(n_sd, SEED_TILE);
  hipLaunchKernelGGL(k_seed_count, dim3(n_tiles), dim3(SDM_BLOCK), 0, ctx->stream, multiplicity,
                     n_sd, s.tile_count);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_seed_scan, dim3(1), dim3(SDM_BLOCK), 0, ctx->stream, s.tile_count,
                     s.tile_offset, (int64_t)n_tiles, seed_index, n_seeds, K, n_sd, ctl, fctl);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_seed_scatter, dim3(n_tiles), dim3(SDM_BLOCK), 0, ctx->stream, idx,
                     multiplicity, (uint64_t *)attributes, n_attr, n_sd, seed_index,
                     seed_multiplicity, (const uint64_t *)seed_attributes, n_seeds, K,
                     s.tile_offset, ctl);
  LAUNCH_CHECK();
  return SDM_OK;
}

}  // namespace

extern "C" int sdm_seeding(sdm_ctx *ctx, int64_t *idx, int64_t *multiplicity,
                           double *extensive_attributes, int64_t n_attr, int64_t n_sd,
                           const int64_t *seeded_particle_index,
                           const int64_t *seeded_particle_multiplicity,
                           const double *seeded_particle_extensive_attributes, int64_t n_seeds,
                           int64_t number_to_inject, int64_t *status) {
  ARG_TRY(ctx && n_attr >= 0 && n_sd >= 0 && n_sd < INT32_MAX && n_seeds >= 0 &&
          number_to_inject >= 0);
  if (number_to_inject == 0) return SDM_OK;
  ARG_TRY(number_to_inject <= n_seeds);
  ARG_TRY(idx && multiplicity && (extensive_attributes || n_attr == 0) && seeded_particle_index &&
          seeded_particle_multiplicity && (seeded_particle_extensive_attributes || n_attr == 0));
  int rc = sdm_reserve(ctx, seed_scratch_bytes(n_sd, 0));
  if (rc) return rc;
  const SeedScratch s = seed_carve(ctx->arena, n_sd, 0);
  static_assert(SEED_GATE < SDM_SEED_STATUS_WORDS, "the gate is a word of the caller's status");
  return inject_async(ctx, s, idx, multiplicity, extensive_attributes, n_attr, n_sd,
                      seeded_particle_index, seeded_particle_multiplicity,
                      seeded_particle_extensive_attributes, n_seeds, number_to_inject,
                      status ? status : s.ctl, nullptr);
}

extern "C" int sdm_seeding_step(sdm_ctx *ctx, int64_t *idx, int64_t *multiplicity,
                                double *extensive_attributes, int64_t n_attr, int64_t n_sd,
                                int64_t *seeded_particle_index,
                                const int64_t *seeded_particle_multiplicity,
                                const double *seeded_particle_extensive_attributes,
                                int64_t n_seeds, int64_t number_to_inject, int shuffle,
                                const uint64_t rng_state_inc[4], uint64_t rng_offset,
                                int64_t *new_length) {
  ARG_TRY(ctx && n_attr >= 0 && n_sd >= 0 && n_sd < INT32_MAX && n_seeds >= 0 &&
          n_seeds < INT32_MAX && number_to_inject >= 0);
  if (number_to_inject == 0) return SDM_OK;
  ARG_TRY(number_to_inject <= n_seeds && new_length);
  ARG_TRY(idx && multiplicity && (extensive_attributes || n_attr == 0) && seeded_particle_index &&
          seeded_particle_multiplicity && (seeded_particle_extensive_attributes || n_attr == 0));
  ARG_TRY(!shuffle || rng_state_inc);
  // the shuffle and the compaction carve the arena from its start, one after the other on the
  // stream; this call's own words lie behind both
  size_t shared = sdm_compact_scratch(n_sd) + 512;
  const size_t shuffle_bytes =
      shuffle ? sdm_shuffle_scratch(n_seeds) + carve_size(sizeof(int64_t) * n_seeds) : 0;
  if (shuffle_bytes > shared) shared = shuffle_bytes;
  shared = carve_size(shared);
  int rc = sdm_reserve(ctx, shared + seed_scratch_bytes(n_sd, n_seeds));
  if (rc) return rc;
  const SeedScratch s = seed_carve(ctx->arena + shared, n_sd, n_seeds);
  if (shuffle && n_seeds > 1) {  // seeding.py:82-88
    rc = sdm_pcg_fill_async(ctx, s.u01, n_seeds, rng_state_inc, rng_offset);
    if (rc) return rc;
    rc = sdm_shuffle_global(ctx, seeded_particle_index, n_seeds, s.u01);
    if (rc) return rc;
  }
  rc = inject_async(ctx, s, nullptr, multiplicity, extensive_attributes, n_attr, n_sd,
                    seeded_particle_index, seeded_particle_multiplicity,
                    seeded_particle_extensive_attributes, n_seeds, number_to_inject, s.ctl,
                    s.fctl);
  if (rc) return rc;
  hipLaunchKernelGGL(k_seed_identity, dim3(grid_for(n_sd)), dim3(SDM_BLOCK), 0, ctx->stream, idx,
                     n_sd, s.ctl);
  LAUNCH_CHECK();
  // sdm_remove_zero_n_or_flagged(multiplicity, idx, n_sd, n_sd) on the block k_seed_scan wrote
  rc = sdm_compact_fused_async(ctx, ctx->arena, multiplicity, idx, n_sd, n_sd, s.fctl, s.cctl,
                               nullptr);
  if (rc) return rc;
  // (ctl, fctl: 256-byte pieces next to each other; 8 words of each)
  HIP_TRY(hipMemcpyAsync(ctx->mailbox, s.ctl, sizeof(int64_t) * 8, hipMemcpyDeviceToHost,
                         ctx->stream));
  HIP_TRY(hipMemcpyAsync(ctx->mailbox + 8, s.fctl, sizeof(int64_t) * 8, hipMemcpyDeviceToHost,
                         ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  const int64_t *status = ctx->mailbox, *fctl = ctx->mailbox + 8;
  if (status[SEED_GATE] == 0) {
    sdm_set_error("seeding: nothing injected: %lld to inject, %lld free slots, %lld seed "
                  "indices outside [0, %lld)", (long long)number_to_inject,
                  (long long)status[SDM_SEED_STATUS_FREE],
                  (long long)status[SDM_SEED_STATUS_BAD_SEED], (long long)n_seeds);
    return SDM_E_STATE;
  }
  if (fctl[7] != 0) {
    (void)sdm_compact_rearm(ctx);
    sdm_set_error("seeding: grid barrier of the compaction kernel timed out");
    return SDM_E_HIP;
  }
  *new_length = fctl[0];
  return SDM_OK;
}
