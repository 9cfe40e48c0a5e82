// collision_pairs.h -- what the kernels of a collision step share about ONE candidate pair: the
// state of a super-droplet as the pair code sees it (SD), the argument block of the fused step
// (FusedArgs), the normalisation factor, the derived radius and fall velocity (derive_ru) and the
// collision probability of a multiplicity-sorted pair (pair_prob_value).  fused.hip's kernels and
// k_parcel_coal (parcel_coal.hip) evaluate a pair through these functions, so that the two agree
// to the bit by construction.  The text is the one fused.hip held before the parcel with
// coalescence needed it in a second translation unit.
#ifndef SDM_COLLISION_PAIRS_H
#define SDM_COLLISION_PAIRS_H
#include "common.h"
#include "physics.h"

// per-super-droplet mirror record: {multiplicity, mass} (16 B) or, when radius / terminal velocity
// are needed (geometric kernel, Berry / Straub breakup), {multiplicity, mass, radius, velocity}
// (32 B): the derived attributes are then evaluated once per change of a droplet instead of once
// per candidate pair and sub-step (attributes/physics/{radius,terminal_velocity}.py semantics)
struct SD { int64_t n; double m, r, u; };
struct Collided;

struct FusedArgs {
  // state
  int64_t *idx;
  int64_t *multiplicity;
  double *attributes;
  const int64_t *cell_id;
  const int64_t *cell_id_raw;  // the caller's cell_id column (== cell_id unless a run relabelled)
  const int64_t *cell_idx;
  const int64_t *cell_start;
  double *dt_left;
  double *stats_dt_min;
  int64_t *stats_n_substep;
  int64_t *collision_rate, *collision_rate_deficit, *coalescence_rate, *breakup_rate,
      *breakup_rate_deficit;
  // the table - or, with a closed-form law (sdm_step_cfg.velocity_law), in the table's place, the
  // law's numbers as sdm_step_state.velocity_params lays them out.  NULL either way = the set-up
  // needs no velocity.  A union, and sdm_step_cfg's two new words fill what was padding in front of
  // this struct: every kernel argument lies where it lay before the laws came, so the table's
  // kernels load their arguments as they did
  union {
    const double *gk_a;
    const double *vel_params;
  };
  const double *gk_b;
  int64_t *ctl;
  // sharded mode (sdm_hip.h): by cell id, 1 = this process computes the cell; NULL = all
  const uint8_t *cell_owned;
  // ... the same by SEGMENT of the permutation (1 = the segment's cell is this process's), written
  // by k_cells_turn for the cell kernel it opens: a workgroup that has nothing to do learns so
  // from one load instead of a chain of four (cell_start -> permutation -> cell id -> mask).  NULL:
  // not available
  const uint8_t *seg_owned;
  // ... and the cell id of every segment (adaptive per-cell route, sharded or not); NULL: unknown
  const int32_t *seg_cid;
  // sharded mode: super-droplets that died in this process's cells in the current sub-step, counted
  // where they are flagged (the list of their positions is built only once the exchange of the
  // counts has shown that somebody's did: k_shard_dead_list); NULL otherwise
  unsigned long long *n_dead;
  // adaptive steps of one cell: the positions of the dead are listed as they are flagged (at most
  // SDM_DEAD_LIST_CAP are kept; the count goes on), for a compaction without a pass over the
  // permutation (index.hip: compact_listed_body); NULL otherwise
  int64_t *dead_pos;
  unsigned long long *dead_count;
  // sharded adaptive per-cell route: minus the deaths per SEGMENT of the permutation (k_cells_turn's
  // min_out + n_cell: completed over the processes by the same all-reduce MIN as the cell minima)
  double *seg_deaths;
  // graph replay (common.h: gwords): s_rand / s_rand_b are then the generators' initial states and
  // the stream positions come from the device ({collision stream, breakup streams}); rand_extra =
  // distance from a draw's first u01 to its first `rand` (n_sd + shift)
  const uint64_t *dev_off;
  uint64_t rand_extra;
  // scratch
  // PCG64 streams, evaluated in the kernels (no u01 arrays): `s_rand` = state of the collision
  // generator at the first draw of `rand` (after pairs_rand), `s_rand_b` = state of the
  // proc_rand / rand_frag generators (same seed, same position: identical values)
  u128 s_rand, s_rand_b, rng_inc;
  const u128 *rng_tab;
  const u128 *rng_aff;  // ready jumps (common.h: pcg_aff); NULL while graph replay is captured
  double *prob;           // [P]
  uint8_t *pair_off;      // [P] 0: pair starts at 2d, 1: at 2d+1, 2: no pair
  int32_t *pair_cid;      // [P] raw cell id of the pair (n_cell > 1)
  double *dt_todo, *cell_min;  // [C]
  double *block_min;           // single cell: per-workgroup partial minima of the optimal dt
  int n_block_min;
  // single adaptive cell, at most 2048 partial minima: k_pair_update does k_cells_adaptive's work
  // itself (0: no; 1: yes; 2: yes, and this is the first sub-step of the time step).  dt_left_pub:
  // dt_left[0] as the previous sub-step left it, in a word nobody writes during this kernel (the
  // compaction's epilogue copies it there)
  int fold_pre;
  const double *dt_left_pub;
  // single-cell fast path: the pair kernels do the shuffle's backward walk themselves (two
  // positions per thread) and write the permuted, pair-sorted idx once; NULL otherwise
  const void *rec;  // records of layout rec_fmt (shuffle_device.h: SDM_REC_*)
  int rec_fmt;
  // inside a call (one cell, non-adaptive, the next step's tile sort riding along): bit 0 = `idx`
  // points to int32_t ids - the next build reads them so - bit 1 = `idx_prev` does; bits 2 and 3:
  // NARROW_TAG_OUT, NARROW_TAG_IN.  (In what was padding: every other member lies where it lay)
  int narrow;
  const int32_t *ovf_head, *ovf_next;
  // successor words: events per tile of the build (shuffle_build.h) when the pair kernels take
  // their workgroups tile by tile (pair_block), 0 = in grid order; tiles the tables are padded to
  int walk_tile, walk_tiles;
  const int64_t *idx_prev;  // previous permutation (source of the dead tail)
  // {multiplicity, mass} of each super-droplet side by side (one random line per gather instead
  // of two); a mirror of the SoA columns kept current by the update code, NULL = not in use
  double *nm;
  int nm_wide;  // 0: 16-B records, 1: 32-B records
  // one cell: every wave of a step would add to the same few counter words, and same-address
  // atomics serialise in L2 (~4 ns each: 70 us per step once most waves hold a colliding pair).
  // The adds go to slot (workgroup % SDM_CNT_SLOTS) instead - one cache line per slot - and
  // k_fold_counters adds the slots to the counters at the end of the call.  NULL: n_cell > 1
  int64_t *slots;
  // breakup: colliding pairs listed by the pair kernels, resolved by k_resolve_dense
  // `list_nl` lists of capacity `list_cap` each (list l starts at list + l * list_cap, its fill
  // count is list_count[l * SDM_CNT_STRIDE]); a workgroup appends to list (blockIdx % list_nl), so
  // the appends of a launch do not all queue up on one counter word
  struct Collided *list;
  unsigned long long *list_count;
  // the fill counts are double-buffered by sub-step: k_resolve_dense clears the set the next
  // sub-step will use (no memset launch per sub-step)
  unsigned long long *list_count_next;
  int list_nl;
  int64_t list_cap;
};

// collisions_methods.py:643-650 (left-to-right evaluation)
__device__ __forceinline__ double norm_factor_of(const sdm_step_cfg &cfg,
                                                 const int64_t *__restrict__ cell_start,
                                                 int64_t c) {
  const int64_t sd_num = cell_start[c + 1] - cell_start[c];
  return sd_num < 2 ? 0.0
                    : cfg.dt / cfg.dv * (double)sd_num * (double)(sd_num - 1) / 2 /
                          (double)(sd_num / 2);
}

// Every kernel that reaches derive_ru exists twice: the instantiation the Gunn-Kinzer law is
// launched with is promised velocity_law == 0 here, first thing, so the closed forms (a pow with
// a run-time exponent: some 25 VGPRs next to the interpolation) are not compiled into it and its
// registers, scratch and occupancy are what they were before the laws came; CLOSED = true is the
// sibling the other laws are launched with.  collision_step() picks by cfg->velocity_law and
// nothing else, so the promise holds.
#define VELOCITY_LAW_PROMISE(CLOSED)                                                \
  do {                                                                              \
    if constexpr (!(CLOSED))                                                        \
      __builtin_assume(cfg.velocity_law == SDM_VELOCITY_LAW_GUNN_KINZER);           \
  } while (0)

// the fall-velocity laws without a table (uniform over the launch; the numbers come through
// scalar loads from a few words every wave shares).  The arithmetic is physics.h's, the one the
// stage kernels k_terminal_velocity / k_power_series run
__device__ __forceinline__ double closed_form_velocity(const sdm_step_cfg &cfg, const FusedArgs &A,
                                                       double r) {
  if (!A.vel_params) return 0.0;
  if (cfg.velocity_law == SDM_VELOCITY_LAW_ROGERS_YAU) return rogers_yau_velocity(r, A.vel_params);
  return power_series_velocity(r, cfg.velocity_terms, A.vel_params,
                               A.vel_params + cfg.velocity_terms);
}

// `id`: the super-droplet `v` is the state of.  With SDM_VELOCITY_MOMENTUM the velocity is the
// reference's `ratio(relative fall momentum, water mass)`, read from the SoA row as it is now (a
// branch uniform over the launch); the radius comes from the mass either way
__device__ __forceinline__ void derive_ru(const sdm_step_cfg &cfg, const FusedArgs &A, SD &v,
                                          int64_t id) {
  const double inv = 1 / (3.14159265358979323846 * 4 / 3);
  v.r = radius_of_volume(volume_of_mass(v.m, cfg.rho_w), inv);
  if (cfg.velocity_source == SDM_VELOCITY_MOMENTUM)
    v.u = (A.attributes + (int64_t)cfg.momentum_attr * cfg.n_sd)[id] / fabs(v.m);
  else if (cfg.velocity_law == SDM_VELOCITY_LAW_GUNN_KINZER)
    v.u = A.gk_a ? gk_interpolate(v.r, cfg.gk_factor, A.gk_a, A.gk_b, cfg.gk_table_len) : 0.0;
  else
    v.u = closed_form_velocity(cfg, A, v.r);
}

// collision probability of one (multiplicity-sorted) pair in slot d: kernel, max multiplicity,
// normalisation (collision.py:249-254; cell of RAW super-droplet #d: reference quirk)
// `norm`: the slot's normalisation factor when the caller has it already (the per-cell kernel
// asks for it ahead of its LDS phases: three dependent look-ups off the critical path), else NULL
template <int KERNEL>
__device__ __forceinline__ double pair_prob_value(const sdm_step_cfg &cfg, const FusedArgs &A,
                                                  int64_t d, const SD &sj, const SD &sk,
                                                  const double *norm = nullptr) {
  const double vj = volume_of_mass(sj.m, cfg.rho_w), vk = volume_of_mass(sk.m, cfg.rho_w);
  double K;
  if (KERNEL == SDM_KERNEL_GOLOVIN) {
    K = (vj + vk) * cfg.kernel_param[0];
  } else if (KERNEL == SDM_KERNEL_GEOMETRIC) {
    const double s = sj.r + sk.r;
    K = (s * s) * cfg.kernel_param[0];
    K *= fabs(sj.u - sk.u);
  } else if (KERNEL == SDM_KERNEL_PARAMETERIZED) {  // parameterized.py:19-30, operation by operation
    const double e = linear_collection_efficiency(cfg.kernel_berry_params, sj.r, sk.r,
                                                  cfg.kernel_berry_unit);
    K = signed_sq(e);
    K *= 3.14159265358979323846;
    const double r_max = sj.r > sk.r ? sj.r : sk.r;
    K *= r_max * r_max;
    K *= fabs(sj.u - sk.u);
  } else if (KERNEL == SDM_KERNEL_SIMPLE_GEOMETRIC) {  // simple_geometric.py:21-27, area.py:14-17
    const double pi_4_3 = 3.14159265358979323846 * 4 / 3;
    const double aj = signed_pow(vj * (1 / pi_4_3), 2.0 / 3.0) * (pi_4_3 * 3);
    const double ak = signed_pow(vk * (1 / pi_4_3), 2.0 / 3.0) * (pi_4_3 * 3);
    const double s = sj.r + sk.r;
    K = cfg.kernel_param[0];
    K *= s * s;
    K *= fabs(aj - ak);
  } else if (KERNEL == SDM_KERNEL_LINEAR) {
    K = (vj + vk) * cfg.kernel_param[1];
    K += cfg.kernel_param[0];
  } else {
    K = cfg.kernel_param[0];
  }
  double prob = (double)sj.n;
  prob *= K;
  prob *= norm ? *norm
               : norm_factor_of(cfg, A.cell_start,
                                cfg.n_cell == 1 ? 0 : A.cell_idx[A.cell_id_raw[d]]);
  return prob;
}

#endif  // SDM_COLLISION_PAIRS_H
