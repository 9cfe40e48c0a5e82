// parcel_coal.hip -- the adiabatic parcel with coalescence (include/sdm_parcel_coal.h, where the
// step is written out): the entry point and k_parcel_coal, the collisions of one time step of
// every parcel.
//
// A step is two launches on the context's stream and no host synchronisation between them:
//   1. a ONE-step launch of k_parcel_p / k_parcel_f_p (parcel_solver.h: parcel_steps over the
//      parcel's permutation and its live rows), which also leaves the step's dv per parcel;
//   2. k_parcel_coal: points 2-4 of the header and the record's row.
//
// k_parcel_coal: one workgroup of 256 lanes per parcel, the workgroups striding over the parcels
// (any grid size is correct; no grid barrier, no residency assumption).  The parcel is ONE cell of
// a collision step, and the whole time step of that cell - every sub-step's shuffle, pairing,
// probability, minimum, gamma and update, the compaction, the adaptive loop - stays inside the
// launch: the permutation, the multiplicities and the three extensive rows are staged in LDS once
// (40 B per row) and written back once; the host polls nothing.  The shuffle is the one of
// fused.hip's per-cell kernel: shuffle_local's events and hit lists, then the backward walks, in
// LDS (16 B per row).  A pair is evaluated by collision_pairs.h (derive_ru, pair_prob_value), the
// functions fused.hip's kernels call, in the same order of operations, and updated by physics.h's
// coalesce_pair on the LDS copy; gamma and the compaction restate collisions_methods.py:522-585,
// 664-680 there (fused.hip's own are written against its global arrays, mirror and counter
// slots), as the shuffle restates the events and walks that k_cell_step holds inline.  Every loop is
// bounded: sub-steps by `substeps` or by the bound the arithmetic sets (sdm_hip.h), walks and the
// compaction by the parcel's rows.
//
// The streams: every parcel has its own PCG64 increment, so the context's jump table (one
// increment) does not apply; a jump is computed from the increment (pcg_affine: the LCG's
// square-and-multiply, at most 64 rounds for the stream position, 12 for a lane's offset in the
// cell).  The position advances by N + N / 2 per sub-step, as sdm_collision_step's does.
//
// Breakup (include/sdm_parcel_breakup.h, sdm_parcel_run_collision): the same kernel with
// BREAKUP = true - see the comment above k_parcel_coal.  The breakup stream is the parcel's own
// generator at rng_offset_breakup[c], one draw per pair slot, advanced by N / 2 per sub-step.
//
// 256 lanes: the flagship shape is 256 rows per parcel - one position per lane in the shuffle and
// one pair per lane of two waves - and 14 KiB of LDS per workgroup, so that the 32-wave limit (8
// workgroups per CU), not LDS, bounds residency; at the cap of 2048 rows a lane owns 8 positions
// and 4 pairs (registers, fixed trip counts) and one workgroup (112 KiB) fits a CU.  The LDS carve
// is sized per call by the largest parcel.
#include <vector>

#include "parcel_solver.h"
#include "collision_pairs.h"
#include "breakup_pairs.h"
#include "../../include/sdm_parcel_coal.h"
#include "../../include/sdm_parcel_breakup.h"

#define PCO_CB 256
#define PCO_ROW_BYTES 56  // int64 + 3 doubles + 5 int32 + 2 int16
#define PCO_MAXPAIR (SDM_PARCEL_COAL_MAX_ROWS / 2 / PCO_CB)
static_assert(SDM_PARCEL_COAL_MAX_ROWS % (2 * PCO_CB) == 0, "pairs per lane");
static_assert(SDM_PARCEL_COAL_MAX_ROWS < 32768, "the hit lists' links are 16-bit");
static_assert(SDM_PARCEL_COAL_MAX_ROWS * PCO_ROW_BYTES <= 150 * 1024, "LDS of one workgroup");

namespace {

struct ParcelCoalArgs {
  int64_t n_parcel, n_sd;
  int64_t at0;  // the first entry of this step's record rows: k * n_parcel
  int64_t max_substeps;
  int cap;  // rows the LDS carve holds
  const int64_t *parcel_start, *failed_step;
  const double *dv;
  double *water_mass, *vdry, *ktdv, *kappa;
  int64_t *multiplicity, *idx, *n_live;
  int64_t *collision_rate, *collision_rate_deficit, *coalescence_rate, *stats_n_substep, *events;
  double *stats_dt_min;
  uint64_t *rng_offset;
  const uint64_t *rng_state_inc;
  sdm_parcel_coal_profile pr;
  // breakup (include/sdm_parcel_breakup.h): read by the BREAKUP instantiations only
  int64_t *breakup_rate, *breakup_rate_deficit;
  uint64_t *rng_offset_breakup;
  sdm_parcel_breakup_profile bpr;
};

// a colliding pair of a sub-step as the breakup branch lists it: 24 B, what the shuffle's tables
// s0, s1 and head hold per PAIR of rows - they are dead once the walks are over
struct PcoCollided { int32_t j, k; double g, u_b; };
static_assert(sizeof(PcoCollided) == 24, "one record in the place of two rows of s0, s1, head");

// (PcgAff, pcg_affine - the jump by `delta` draws as an affine map: parcel_solver.h, which the
// mixed-phase parcel's kernels use too)

// BREAKUP: the step of include/sdm_parcel_breakup.h with enable_breakup - a colliding pair bounces,
// coalesces or breaks up.  The pair loop only LISTS the colliding pairs {j, k, gamma, u_b} in LDS
// (the efficiencies and fragmentations are transcendental-heavy and colliding pairs are rare:
// inlined PCO_MAXPAIR times into the unrolled loop they would cost every lane their registers), and
// all lanes then stride over the list and resolve it densely - k_resolve_dense's idea inside one
// workgroup.  The resolution restates fused.hip's resolve_collision<true> on the LDS copy.  The
// instantiations sdm_parcel_run_coal launches are the BREAKUP = false ones, as they were.
template <int KERNEL, bool CLOSED, bool BREAKUP>
__global__ void __launch_bounds__(PCO_CB)
k_parcel_coal(sdm_step_cfg cfg, FusedArgs A, ParcelCoalArgs a) {
  VELOCITY_LAW_PROMISE(CLOSED);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int R = a.cap;
  int64_t *s_n = (int64_t *)smem;     // [R] multiplicity by relative row; -1: not staged
  double *s_x = (double *)(s_n + R);  // [3][R] water mass, dry volume, kappa times dry volume
  int32_t *val = (int32_t *)(s_x + 3 * R), *out = val + R;  // the permutation (relative rows)
  int32_t *s0 = out + R, *s1 = s0 + R, *head = s1 + R;      // the shuffle's hit tables
  int16_t *jown = (int16_t *)(head + R), *next = jown + R;
  __shared__ double red[PCO_CB / SDM_WAVE];
  __shared__ int s_died, s_valid, s_bad;
  // [3 ..]: breakup_rate, breakup_rate_deficit, n_overflow of the step; the fill of the pair list
  __shared__ unsigned long long s_cnt[BREAKUP ? 7 : 3];
  PcoCollided *const list = (PcoCollided *)s0;  // [R / 2], BREAKUP only (see PcoCollided)
  const int tid = (int)threadIdx.x;
  const bool need_r = KERNEL == SDM_KERNEL_GEOMETRIC || KERNEL == SDM_KERNEL_PARAMETERIZED ||
                      KERNEL == SDM_KERNEL_SIMPLE_GEOMETRIC;
  for (int64_t c = blockIdx.x; c < a.n_parcel; c += gridDim.x) {
    const int64_t row0 = a.parcel_start[c], rows = a.parcel_start[c + 1] - row0;
    // (checked on the host too; a failed parcel is left alone for good.  Uniform over the workgroup)
    if (row0 < 0 || rows <= 0 || row0 + rows > a.n_sd || rows > R || a.failed_step[c] >= 0)
      continue;
    const int N = (int)rows;
    const int live0 = (int)a.n_live[c];
    if (live0 < 1 || live0 > N) continue;
    __syncthreads();  // the previous parcel's reads of LDS are over
    if (tid == 0) {
      s_died = 0;
      s_bad = 0;
      s_valid = live0;
      s_cnt[0] = s_cnt[1] = s_cnt[2] = 0;
      if constexpr (BREAKUP) s_cnt[3] = s_cnt[4] = s_cnt[5] = s_cnt[6] = 0;
    }
    for (int q = tid; q < N; q += PCO_CB) s_n[q] = -1;
    __syncthreads();
    // ---- staging: the rows of the live positions ------------------------------------------------
    for (int p = tid; p < live0; p += PCO_CB) {
      const int64_t rel = a.idx[row0 + p] - row0;
      if (rel < 0 || rel >= N) {  // (the host checks a fresh permutation; the kernel keeps it valid)
        s_bad = 1;
        continue;
      }
      const int64_t row = row0 + rel;
      val[p] = (int32_t)rel;
      s_n[rel] = a.multiplicity[row];
      s_x[rel] = a.water_mass[row];
      s_x[R + rel] = a.vdry[row];
      s_x[2 * R + rel] = a.ktdv[row];
    }
    __syncthreads();
    if (s_bad) continue;  // (uniform)
    const double dv = a.dv[c];
    cfg.dv = dv;  // (the kernel's own copy of the set-up: norm_factor_of reads it)
    const int64_t n_sub_before = a.stats_n_substep[c];
    int64_t stats_n = n_sub_before;
    double stats_min = a.stats_dt_min[c];
    int64_t event = 0, subs = 0;
    int64_t rate = 0, deficit = 0, coalesced = 0;  // this lane's share of the step's counts
    int64_t broken = 0, broken_deficit = 0, overflows = 0;  // (BREAKUP)
    uint64_t drawn = 0, drawn_b = 0;
    int valid = live0;
    if (N >= 2) {
      const u128 inc = (((u128)a.rng_state_inc[4 * c + 2]) << 64) | a.rng_state_inc[4 * c + 3];
      u128 base = (((u128)a.rng_state_inc[4 * c]) << 64) | a.rng_state_inc[4 * c + 1];
      {  // the stream at this parcel's position (uniform: every lane computes it)
        const PcgAff to_now = pcg_affine(inc, a.rng_offset[c]);
        base = base * to_now.m + to_now.p;
      }
      u128 base_b = 0;  // BREAKUP: the same generator at the position of the proc / frag stream
      if constexpr (BREAKUP) {
        const PcgAff to_now = pcg_affine(inc, a.rng_offset_breakup[c]);
        base_b = ((((u128)a.rng_state_inc[4 * c]) << 64) | a.rng_state_inc[4 * c + 1]) * to_now.m +
                 to_now.p;
      }
      const int P = N / 2;
      const PcgAff over_u01 = pcg_affine(inc, (uint64_t)N);        // u01 window -> `rand`
      const PcgAff over_rand = pcg_affine(inc, (uint64_t)P);       // `rand` -> next sub-step
      double dt_left = cfg.dt;
#pragma unroll 1
      for (;;) {
        if (cfg.adaptive) {  // (all of this is uniform over the workgroup)
          if (dt_left == 0) break;
          if (subs > a.max_substeps) {  // where sdm_collision_step returns SDM_E_STATE
            event |= SDM_PARCEL_COAL_EVENT_BOUND;
            break;
          }
        } else if (subs >= cfg.substeps) {
          break;
        }
        const int n = valid;
        // ---- shuffle_local (index_methods.py:32-43): events, then backward walks ------------------
        for (int li = tid; li < n; li += PCO_CB) {
          s0[li] = -1; s1[li] = -1; head[li] = -1;
        }
        if constexpr (BREAKUP) {  // (the last sub-step's list was read before its closing barrier)
          if (tid == 0) s_cnt[6] = 0;
        }
        __syncthreads();
        {
          const int chunk = (n + PCO_CB - 1) / PCO_CB;
          const int li0 = tid * chunk;
          if (li0 < n) {
            const PcgAff to_me = pcg_affine(inc, (uint64_t)li0);
            u128 state = base * to_me.m + to_me.p;
            const u128 mult = pcg_mult();
            for (int e = 0; e < chunk && li0 + e < n; ++e) {
              const int li = li0 + e;
              state = state * mult + inc;
              const double u = pcg_output(state);
              int jt = -1;
              if (li > 0) {
                const int64_t t = (int64_t)((double)0 + u * (double)n);
                jt = (int)(t > n - 1 ? n - 1 : (t < 0 ? 0 : t));
                if (atomicCAS(&s0[jt], -1, li) != -1)
                  if (atomicCAS(&s1[jt], -1, li) != -1)
                    next[li] = (int16_t)atomicExch(&head[jt], li);
              }
              jown[li] = (int16_t)jt;
            }
          }
        }
        __syncthreads();
        for (int li = tid; li < n; li += PCO_CB) {
          int e = 0, q = li;
          for (;;) {
            int best = INT32_MAX;
            const int jq = jown[q];
            if (q > e && jq >= 0) best = q;
            const int h0 = s0[q], h1 = s1[q];
            if (h0 > e && h0 < best) best = h0;
            if (h1 > e && h1 < best) best = h1;
            for (int t = head[q]; t >= 0; t = next[t])
              if (t > e && t < best) best = t;
            if (best == INT32_MAX) break;
            q = (best == q) ? jq : best;
            e = best;
          }
          out[li] = val[q];
        }
        __syncthreads();
        // ---- pairs, sort within pair, probability (collision.py:249-271) ---------------------------
        const int n_pairs = n / 2;
        const int pchunk = (n_pairs + PCO_CB - 1) / PCO_CB;  // <= PCO_MAXPAIR
        const int d0 = tid * pchunk;
        const int64_t one_cell[2] = {0, n};
        const double norm = norm_factor_of(cfg, one_cell, 0);  // (cfg.dv: this parcel's, this step's)
        int pj[PCO_MAXPAIR], pk[PCO_MAXPAIR];
        int64_t pnj[PCO_MAXPAIR], pnk[PCO_MAXPAIR];
        double pprob[PCO_MAXPAIR];
        bool pvalid[PCO_MAXPAIR];
        double my_min = INFINITY;
#pragma unroll
        for (int r = 0; r < PCO_MAXPAIR; ++r) {
          const int d = d0 + r;
          pvalid[r] = r < pchunk && d < n_pairs;
          pj[r] = pk[r] = 0;
          pnj[r] = pnk[r] = 1;
          pprob[r] = 0.0;
          if (!pvalid[r]) continue;
          int j = out[2 * d], k = out[2 * d + 1];
          SD sj, sk;
          sj.n = s_n[j]; sj.m = s_x[j]; sj.r = sj.u = 0.0;
          sk.n = s_n[k]; sk.m = s_x[k]; sk.r = sk.u = 0.0;
          if (sj.n < sk.n) {  // sort_within_pair_by_attr
            const int t = j; j = k; k = t;
            const SD ts = sj; sj = sk; sk = ts;
            out[2 * d] = j;
            out[2 * d + 1] = k;
          }
          if (need_r) {
            derive_ru(cfg, A, sj, j);
            derive_ru(cfg, A, sk, k);
          }
          const double prob = pair_prob_value<KERNEL>(cfg, A, d, sj, sk, &norm);
          pj[r] = j; pk[r] = k;
          pnj[r] = sj.n; pnk[r] = sk.n;
          pprob[r] = prob;
          if (cfg.adaptive && prob != 0) {
            const int64_t prop = sj.n / sk.n;
            const double t = cfg.dt * (double)prop / prob;
            const double dt_opt = cfg.dt_min > t ? cfg.dt_min : t;
            my_min = dt_opt < my_min ? dt_opt : my_min;
          }
        }
        double scale = 1.0;
        if (cfg.adaptive) {  // collisions_methods.py:355-374 for the one cell
          const double m = wave_min_f64(my_min);
          if ((tid & 63) == 0) red[tid >> 6] = m;
          __syncthreads();
          double bmin = red[0];
          for (int w = 1; w < PCO_CB / SDM_WAVE; ++w) bmin = red[w] < bmin ? red[w] : bmin;
          double todo = cfg.dt_max < dt_left ? cfg.dt_max : dt_left;
          if (bmin < todo) todo = bmin;
          if (bmin < stats_min) stats_min = bmin;  // (a NaN stays, as in the reference)
          if (stats_min == cfg.dt_min) event |= SDM_PARCEL_COAL_EVENT_DT_MIN;
          scale = todo / cfg.dt;
          dt_left -= todo;
          if (todo > 0) stats_n += 1;
        }
        // ---- gamma and the update (collisions_methods.py:522-585, 44-59) ---------------------------
        {
          const u128 rand0 = base * over_u01.m + over_u01.p;
          const PcgAff to_me = pcg_affine(inc, (uint64_t)d0);
          u128 st = rand0 * to_me.m + to_me.p;
          u128 sb = 0;  // one draw per pair slot: the efficiency decision and the fragmentation
          if constexpr (BREAKUP) sb = base_b * to_me.m + to_me.p;
#pragma unroll
          for (int r = 0; r < PCO_MAXPAIR; ++r) {
            st = st * pcg_mult() + inc;
            if constexpr (BREAKUP) sb = sb * pcg_mult() + inc;
            if (!pvalid[r]) continue;
            const double u = pcg_output(st);
            double p = pprob[r];
            if (p != 0) {
              if (cfg.adaptive) p *= scale;
              else p /= (double)cfg.substeps;
            }
            double g = ceil(p - u);
            if (g == 0) continue;
            const int64_t nj = pnj[r], nk = pnk[r];
            const int64_t prop = nj / nk;
            const int64_t gi = (int64_t)g;
            const int64_t gc = gi < prop ? gi : prop;
            rate += gc * nk;
            deficit += (gi - gc) * nk;
            g = (double)gc;
            if (g == 0) continue;
            const int j = pj[r], k = pk[r];
            if constexpr (BREAKUP) {  // listed; resolved below (at most n / 2 records: they fit)
              const int at = (int)atomicAdd(&s_cnt[6], 1ull);
              PcoCollided rec;
              rec.j = j; rec.k = k; rec.g = g; rec.u_b = pcg_output(sb);
              list[at] = rec;
              continue;
            }
            coalesced += (int64_t)(g * (double)nk);
            coalesce_pair(j, k, g, s_n, s_x, 3, R);  // (physics.h, on the LDS copy)
            if (s_n[j] == 0 || s_n[k] == 0) s_died = 1;  // flag_zero_multiplicity
          }
        }
        if constexpr (BREAKUP) {
          // ---- bounce, coalescence or breakup of the listed pairs (collisions_methods.py:247-311;
          // fused.hip: resolve_collision<true>, on the LDS copy).  The pairs of a sub-step are
          // disjoint and the counters integer sums: the result does not depend on the list's order
          __syncthreads();
          const int n_coll = (int)s_cnt[6];  // <= n_pairs
          const bool need_ru = cfg.ec != SDM_EC_CONST || cfg.frag == SDM_FRAG_STRAUB2010 ||
                               cfg.frag == SDM_FRAG_LOWLIST1982;
          for (int t = tid; t < n_coll; t += PCO_CB) {
            const PcoCollided rec = list[t];
            int j = rec.j, k = rec.k;
            const int j_in = j, k_in = k;
            const double g = rec.g, u_b = rec.u_b;
            const int64_t nk = s_n[k];
            double ec, fm;
            {  // radius and velocity on demand: there is no mirror record in LDS
              SD sj, sk;
              sj.n = s_n[j]; sj.m = s_x[j]; sj.r = sj.u = 0.0;
              sk.n = nk; sk.m = s_x[k]; sk.r = sk.u = 0.0;
              if (need_ru) {
                derive_ru(cfg, A, sj, j);
                derive_ru(cfg, A, sk, k);
              }
              breakup_params(cfg, A, sj, sk, u_b, ec, fm);
            }
            if (u_b - (ec + (1 - ec) * cfg.eb_const) > 0) continue;  // bounce
            if (u_b - ec < 0) {
              coalesced += (int64_t)(g * (double)nk);
              coalesce_pair(j, k, g, s_n, s_x, 3, R);
            } else {
              bool ovf = false;
              const double *mass = s_x;  // (mass_attr = 0)
              // break_up / break_up_while (collisions_methods.py:135-243)
              double gamma_deficit = g;
              if (!cfg.handle_all_breakups) {
                double take_from_j, new_mult_k;
                int64_t gamma_j_k;
                compute_transfer_multiplicities(g, s_n[j], nk, mass[j], mass[k], fm,
                                                cfg.max_multiplicity, take_from_j, new_mult_k,
                                                gamma_j_k, ovf);
                gamma_deficit = g - (double)gamma_j_k;
                broken += gamma_j_k * nk;
                if (gamma_deficit != 0) broken_deficit += (int64_t)(gamma_deficit * (double)nk);
                apply_breakup_transfer(j, k, take_from_j, new_mult_k, s_n, s_x, 3, R);
              } else {
                // (bounded: every pass but the last takes at least 1 from gamma_deficit - the
                // g_int == 0 exit of fused.hip, where the reference's loop would never end)
                while (gamma_deficit > 0) {
                  double take_from_j, new_mult_k, gamma_j_k;
                  const int64_t mj = s_n[j], mk = s_n[k];
                  if (mk == mj) {
                    take_from_j = (double)mj;
                    new_mult_k = (mass[j] + mass[k]) / fm * (double)mk;
                    if (new_mult_k > (double)cfg.max_multiplicity) {
                      broken_deficit += (int64_t)(gamma_deficit * (double)mk);
                      ovf = true;
                      break;
                    }
                    gamma_j_k = gamma_deficit;
                  } else {
                    if (mk > mj) { const int t2 = j; j = k; k = t2; }
                    int64_t g_int;
                    compute_transfer_multiplicities(gamma_deficit, s_n[j], s_n[k], mass[j],
                                                    mass[k], fm, cfg.max_multiplicity, take_from_j,
                                                    new_mult_k, g_int, ovf);
                    gamma_j_k = (double)g_int;
                    if (g_int == 0) break;
                  }
                  broken += (int64_t)(gamma_j_k * (double)s_n[k]);
                  gamma_deficit -= gamma_j_k;
                  apply_breakup_transfer(j, k, take_from_j, new_mult_k, s_n, s_x, 3, R);
                }
                broken_deficit += (int64_t)(gamma_deficit * (double)s_n[k]);
              }
              overflows += ovf ? 1 : 0;
            }
            if (s_n[j_in] == 0 || s_n[k_in] == 0) s_died = 1;  // flag_zero_multiplicity
          }
          base_b = base_b * over_rand.m + over_rand.p;
          drawn_b += (uint64_t)P;
        }
        base = (base * over_u01.m + over_u01.p) * over_rand.m + over_rand.p;
        drawn += (uint64_t)(N + P);
        subs += 1;
        __syncthreads();
        // ---- the compaction (collisions_methods.py:664-680), where somebody died ------------------
        if (s_died) {  // (uniform: nobody clears it before the next barrier)
          __syncthreads();
          if (tid == 0) {
            int new_length = n, i = 0;
            while (i < new_length) {
              if (s_n[out[i]] == 0) {
                new_length -= 1;
                out[i] = out[new_length];
                out[new_length] = N;
              } else {
                i += 1;
              }
            }
            s_valid = new_length;
            s_died = 0;
          }
          __syncthreads();
          valid = s_valid;
        }
        for (int li = tid; li < valid; li += PCO_CB) val[li] = out[li];
        // (the next sub-step's barriers come before anybody reads val or writes out again)
      }
      __syncthreads();
    }
    // ---- write-back: the rows that were staged; kappa of those that live (point 3) ----------------
    for (int q = tid; q < N; q += PCO_CB) {
      const int64_t n_q = s_n[q];
      if (n_q < 0) continue;
      const int64_t row = row0 + q;
      a.multiplicity[row] = n_q;
      a.water_mass[row] = s_x[q];
      const double vd = s_x[R + q], kt = s_x[2 * R + q];
      a.vdry[row] = vd;
      a.ktdv[row] = kt;
      if (n_q > 0) a.kappa[row] = kt / vd;
    }
    for (int p = tid; p < valid; p += PCO_CB) a.idx[row0 + p] = row0 + val[p];
    {  // the step's counts: one LDS atomic per wave, then lane 0
      const int64_t r = wave_sum_i64(rate), d = wave_sum_i64(deficit), k = wave_sum_i64(coalesced);
      if (lane_id() == 0) {
        if (r) atomicAdd(&s_cnt[0], (unsigned long long)r);
        if (d) atomicAdd(&s_cnt[1], (unsigned long long)d);
        if (k) atomicAdd(&s_cnt[2], (unsigned long long)k);
      }
      if constexpr (BREAKUP) {
        const int64_t b = wave_sum_i64(broken), bd = wave_sum_i64(broken_deficit),
                      o = wave_sum_i64(overflows);
        if (lane_id() == 0) {
          if (b) atomicAdd(&s_cnt[3], (unsigned long long)b);
          if (bd) atomicAdd(&s_cnt[4], (unsigned long long)bd);
          if (o) atomicAdd(&s_cnt[5], (unsigned long long)o);
        }
      }
    }
    __syncthreads();
    if (tid == 0) {
      a.n_live[c] = valid;
      a.collision_rate[c] += (int64_t)s_cnt[0];
      a.collision_rate_deficit[c] += (int64_t)s_cnt[1];
      a.coalescence_rate[c] += (int64_t)s_cnt[2];
      a.stats_n_substep[c] = stats_n;
      a.stats_dt_min[c] = stats_min;
      if (event) a.events[c] |= event;
      a.rng_offset[c] += drawn;
      if constexpr (BREAKUP) {
        a.breakup_rate[c] += (int64_t)s_cnt[3];
        a.breakup_rate_deficit[c] += (int64_t)s_cnt[4];
        if (s_cnt[5]) a.events[c] += (int64_t)(s_cnt[5] << SDM_PARCEL_COAL_OVERFLOW_SHIFT);
        a.rng_offset_breakup[c] += drawn_b;
      }
      const int64_t at = a.at0 + c;
      if (a.pr.n_live) a.pr.n_live[at] = valid;
      if (a.pr.n_substeps) a.pr.n_substeps[at] = subs;
      if (a.pr.coalescence_rate) a.pr.coalescence_rate[at] = (int64_t)s_cnt[2];
      if (a.pr.collision_rate_deficit) a.pr.collision_rate_deficit[at] = (int64_t)s_cnt[1];
      if (a.pr.dv) a.pr.dv[at] = dv;
      if constexpr (BREAKUP) {
        if (a.bpr.breakup_rate) a.bpr.breakup_rate[at] = (int64_t)s_cnt[3];
        if (a.bpr.breakup_rate_deficit) a.bpr.breakup_rate_deficit[at] = (int64_t)s_cnt[4];
        if (a.bpr.n_overflow) a.bpr.n_overflow[at] = (int64_t)s_cnt[5];
      }
    }
  }
}

// the step's dv per parcel (n_parcel doubles) in the buffer parcel_chem.hip keeps its own in: no
// call leaves anything there for a later one
int reserve_dv(sdm_ctx *ctx, size_t bytes) {
  if (bytes <= ctx->parcel_chem_bytes) return SDM_OK;
  HIP_TRY(hipStreamSynchronize(ctx->stream));  // earlier launches may still use the old one
  if (ctx->parcel_chem_buf) HIP_TRY(hipFree(ctx->parcel_chem_buf));
  ctx->parcel_chem_buf = nullptr;
  ctx->parcel_chem_bytes = 0;
  const size_t want = bytes + bytes / 4 + 4096;
  if (hipMalloc((void **)&ctx->parcel_chem_buf, want) != hipSuccess) {
    sdm_set_error("sdm_parcel_run_coal: hipMalloc(%zu) failed", want);
    return SDM_E_NOMEM;
  }
  ctx->parcel_chem_bytes = want;
  return SDM_OK;
}

template <int KERNEL, bool CLOSED, bool BREAKUP>
int launch_coal(sdm_ctx *ctx, unsigned grid, size_t lds, const sdm_step_cfg &cfg,
                const FusedArgs &A, const ParcelCoalArgs &a) {
  hipLaunchKernelGGL((k_parcel_coal<KERNEL, CLOSED, BREAKUP>), dim3(grid), dim3(PCO_CB), lds,
                     ctx->stream, cfg, A, a);
  LAUNCH_CHECK();
  return SDM_OK;
}
template <int KERNEL, bool CLOSED, bool BREAKUP>
int allow_lds(size_t lds) {  // large dynamic LDS must be opted into, per kernel (the caller asks
                             // from 48 KiB on, below any limit a runtime may apply)
  HIP_TRY(hipFuncSetAttribute((const void *)k_parcel_coal<KERNEL, CLOSED, BREAKUP>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return SDM_OK;
}

#define COAL_DISPATCH(FN, B, ...)                                                               \
  ([&]() -> int {                                                                               \
    switch (kc.kernel * 2 + (closed ? 1 : 0)) {                                                 \
      case SDM_KERNEL_GOLOVIN * 2:                                                              \
        return FN<SDM_KERNEL_GOLOVIN, false, B>(__VA_ARGS__);                                   \
      case SDM_KERNEL_GOLOVIN * 2 + 1:                                                          \
        return FN<SDM_KERNEL_GOLOVIN, true, B>(__VA_ARGS__);                                    \
      case SDM_KERNEL_GEOMETRIC * 2:                                                            \
        return FN<SDM_KERNEL_GEOMETRIC, false, B>(__VA_ARGS__);                                 \
      case SDM_KERNEL_GEOMETRIC * 2 + 1:                                                        \
        return FN<SDM_KERNEL_GEOMETRIC, true, B>(__VA_ARGS__);                                  \
      case SDM_KERNEL_CONSTANT * 2:                                                             \
        return FN<SDM_KERNEL_CONSTANT, false, B>(__VA_ARGS__);                                  \
      case SDM_KERNEL_CONSTANT * 2 + 1:                                                         \
        return FN<SDM_KERNEL_CONSTANT, true, B>(__VA_ARGS__);                                   \
      case SDM_KERNEL_PARAMETERIZED * 2:                                                        \
        return FN<SDM_KERNEL_PARAMETERIZED, false, B>(__VA_ARGS__);                             \
      case SDM_KERNEL_PARAMETERIZED * 2 + 1:                                                    \
        return FN<SDM_KERNEL_PARAMETERIZED, true, B>(__VA_ARGS__);                              \
      case SDM_KERNEL_SIMPLE_GEOMETRIC * 2:                                                     \
        return FN<SDM_KERNEL_SIMPLE_GEOMETRIC, false, B>(__VA_ARGS__);                          \
      case SDM_KERNEL_SIMPLE_GEOMETRIC * 2 + 1:                                                 \
        return FN<SDM_KERNEL_SIMPLE_GEOMETRIC, true, B>(__VA_ARGS__);                           \
      case SDM_KERNEL_LINEAR * 2:                                                               \
        return FN<SDM_KERNEL_LINEAR, false, B>(__VA_ARGS__);                                    \
      default:                                                                                  \
        return FN<SDM_KERNEL_LINEAR, true, B>(__VA_ARGS__);                                     \
    }                                                                                           \
  })()

}  // namespace

// both entry points; `who` names the one that was called.  `breakup` / `breakup_profile` are read
// only with coal_cfg->enable_breakup (include/sdm_parcel_breakup.h)
static int parcel_run_collision(
    const char *who, sdm_ctx *ctx, const sdm_parcel_cfg *cfg, const sdm_step_cfg *coal_cfg,
    int64_t n_steps, int64_t n_parcel, int64_t n_sd, const int64_t *parcel_start,
    double *water_mass, int64_t *multiplicity, double *vdry, double *kappa, const double *f_org,
    double *v_cr, const sdm_parcel_state *state, const double *w_mid,
    const sdm_parcel_profile *profile, const double consts[34], const sdm_cond_formulae *formulae,
    const sdm_parcel_coal_state *coal, const sdm_parcel_coal_profile *coal_profile, int fresh_idx,
    const sdm_parcel_breakup_state *breakup, const sdm_parcel_breakup_profile *breakup_profile) {
  // what this route does not serve
  ARG_TRY(!coal_cfg->optimized_random);
  ARG_TRY(coal_cfg->croupier_local);
  ARG_TRY(coal_cfg->velocity_source == SDM_VELOCITY_TERMINAL);
  // ... and the checks of sdm_collision_step
  const int law = coal_cfg->velocity_law;
  ARG_TRY(law >= SDM_VELOCITY_LAW_GUNN_KINZER && law <= SDM_VELOCITY_LAW_POWER_SERIES);
  ARG_TRY(law != SDM_VELOCITY_LAW_POWER_SERIES ||
          (coal_cfg->velocity_terms >= 0 && coal_cfg->velocity_terms <= SDM_VELOCITY_MAX_TERMS));
  ARG_TRY(coal_cfg->kernel >= SDM_KERNEL_GOLOVIN && coal_cfg->kernel <= SDM_KERNEL_LINEAR);
  const bool with_breakup = coal_cfg->enable_breakup != 0;
  if (with_breakup) {
    ARG_TRY(coal_cfg->ec >= SDM_EC_CONST && coal_cfg->ec <= SDM_EC_LOWLIST1982);
    ARG_TRY(coal_cfg->frag >= SDM_FRAG_ALWAYS_N && coal_cfg->frag <= SDM_FRAG_LOWLIST1982);
    ARG_TRY(coal_cfg->max_multiplicity >= 1);
  }
  // (the set-up needs a fall velocity: the kernel does, or an efficiency / fragmentation that
  // forms the pair's kinetic energy)
  const bool kernel_needs_velocity =
      coal_cfg->kernel == SDM_KERNEL_GEOMETRIC || coal_cfg->kernel == SDM_KERNEL_PARAMETERIZED ||
      (with_breakup &&
       (coal_cfg->ec == SDM_EC_STRAUB2010 || coal_cfg->ec == SDM_EC_LOWLIST1982 ||
        coal_cfg->frag == SDM_FRAG_STRAUB2010 || coal_cfg->frag == SDM_FRAG_LOWLIST1982));
  ARG_TRY(law != SDM_VELOCITY_LAW_GUNN_KINZER || !kernel_needs_velocity ||
          (coal->gk_a && coal->gk_b && coal_cfg->gk_table_len > 0));
  ARG_TRY(law == SDM_VELOCITY_LAW_GUNN_KINZER || !kernel_needs_velocity ||
          coal->velocity_params ||
          (law == SDM_VELOCITY_LAW_POWER_SERIES && coal_cfg->velocity_terms == 0));
  ARG_TRY(coal_cfg->adaptive || coal_cfg->substeps >= 1);
  ARG_TRY(!(coal_cfg->dt_min <= 0));
  ARG_TRY(!coal_cfg->adaptive || coal_cfg->dt_min == coal_cfg->dt_min);
  ParcelCall call;
  bool with_diag, nothing_to_do;
  const int prepared = sdm_parcel_prepare(ctx, cfg, n_steps, n_parcel, n_sd, parcel_start,
                                          water_mass, multiplicity, vdry, kappa, f_org, v_cr, state,
                                          w_mid, profile, consts, formulae, nullptr, nullptr, &call,
                                          &with_diag, &nothing_to_do);
  if (prepared != SDM_OK || nothing_to_do) return prepared;
  ARG_TRY(coal->idx && coal->n_live && coal->kappa_times_dry_volume && coal->collision_rate &&
          coal->collision_rate_deficit && coal->coalescence_rate && coal->stats_n_substep &&
          coal->stats_dt_min && coal->events && coal->rng_offset && coal->rng_state_inc);
  ARG_TRY(!with_breakup || (breakup && breakup->breakup_rate && breakup->breakup_rate_deficit &&
                            breakup->rng_offset_breakup));

  // the parcels' sizes (sdm_parcel_prepare has checked that they are positive and lie in the columns)
  std::vector<int64_t> starts((size_t)n_parcel + 1);
  HIP_TRY(hipMemcpyAsync(starts.data(), parcel_start, starts.size() * sizeof(int64_t),
                         hipMemcpyDeviceToHost, ctx->stream));
  std::vector<int64_t> live, perm;
  if (fresh_idx) {
    live.resize((size_t)n_parcel);
    perm.resize((size_t)n_sd);
    HIP_TRY(hipMemcpyAsync(live.data(), coal->n_live, live.size() * sizeof(int64_t),
                           hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(perm.data(), coal->idx, perm.size() * sizeof(int64_t),
                           hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  int64_t most = 0;
  for (int64_t c = 0; c < n_parcel; ++c) {
    const int64_t row0 = starts[(size_t)c], rows = starts[(size_t)c + 1] - row0;
    if (rows > SDM_PARCEL_COAL_MAX_ROWS) {
      sdm_set_error("%s: parcel %lld has %lld rows, more than SDM_PARCEL_COAL_MAX_ROWS = %d", who,
                    (long long)c, (long long)rows, SDM_PARCEL_COAL_MAX_ROWS);
      return SDM_E_ARG;
    }
    most = rows > most ? rows : most;
    if (!fresh_idx) continue;
    const int64_t n = live[(size_t)c];
    if (n < 1 || n > rows) {
      sdm_set_error("%s: n_live[%lld] = %lld is outside 1 .. %lld", who, (long long)c,
                    (long long)n, (long long)rows);
      return SDM_E_ARG;
    }
    for (int64_t p = 0; p < n; ++p) {
      const int64_t row = perm[(size_t)(row0 + p)];
      if (row < row0 || row >= row0 + rows) {
        sdm_set_error("%s: idx[%lld] = %lld is outside the rows of parcel %lld", who,
                      (long long)(row0 + p), (long long)row, (long long)c);
        return SDM_E_ARG;
      }
    }
  }
  const int reserved = reserve_dv(ctx, carve_size(sizeof(double) * (size_t)n_parcel));
  if (reserved != SDM_OK) return reserved;
  double *dv = (double *)ctx->parcel_chem_buf;

  sdm_step_cfg kc = *coal_cfg;
  kc.n_cell = 1;
  kc.n_attr = 3;
  kc.mass_attr = 0;
  kc.dt = cfg->dt;
  const bool closed = law != SDM_VELOCITY_LAW_GUNN_KINZER;
  FusedArgs A;
  memset(&A, 0, sizeof(A));
  if (closed) {
    A.vel_params = coal->velocity_params;
  } else {
    A.gk_a = coal->gk_a;
    A.gk_b = coal->gk_b;
  }
  ParcelCoalArgs a;
  a.n_parcel = n_parcel;
  a.n_sd = n_sd;
  a.max_substeps = INT64_MAX;
  if (kc.adaptive) {  // the bound of sdm_collision_step (sdm_hip.h)
    const double q = kc.dt / kc.dt_min;
    a.max_substeps = q < 4e18 ? (int64_t)ceil(q) + 2 : INT64_MAX;
  }
  a.cap = (int)((most + 63) / 64 * 64);
  a.parcel_start = parcel_start;
  a.failed_step = state->failed_step;
  a.dv = dv;
  a.water_mass = water_mass;
  a.vdry = vdry;
  a.ktdv = coal->kappa_times_dry_volume;
  a.kappa = kappa;
  a.multiplicity = multiplicity;
  a.idx = coal->idx;
  a.n_live = coal->n_live;
  a.collision_rate = coal->collision_rate;
  a.collision_rate_deficit = coal->collision_rate_deficit;
  a.coalescence_rate = coal->coalescence_rate;
  a.stats_n_substep = coal->stats_n_substep;
  a.events = coal->events;
  a.stats_dt_min = coal->stats_dt_min;
  a.rng_offset = coal->rng_offset;
  a.rng_state_inc = coal->rng_state_inc;
  if (coal_profile) a.pr = *coal_profile;
  else memset(&a.pr, 0, sizeof(a.pr));
  a.breakup_rate = a.breakup_rate_deficit = nullptr;
  a.rng_offset_breakup = nullptr;
  memset(&a.bpr, 0, sizeof(a.bpr));
  if (with_breakup) {
    a.breakup_rate = breakup->breakup_rate;
    a.breakup_rate_deficit = breakup->breakup_rate_deficit;
    a.rng_offset_breakup = breakup->rng_offset_breakup;
    if (breakup_profile) a.bpr = *breakup_profile;
  }
  const size_t lds = (size_t)a.cap * PCO_ROW_BYTES;
  if (lds > 48 * 1024) {
    const int allowed = with_breakup ? COAL_DISPATCH(allow_lds, true, lds)
                                     : COAL_DISPATCH(allow_lds, false, lds);
    if (allowed != SDM_OK) return allowed;
  }
  call.identity = coal->idx;  // the parcel kernels follow the caller's permutation
  const unsigned grid =
      (unsigned)(n_parcel < SDM_PARCEL_COAL_MAX_GRID ? n_parcel : SDM_PARCEL_COAL_MAX_GRID);
  for (int64_t step = 0; step < n_steps; ++step) {
    call.k0 = step;
    call.k_count = 1;
    const int launched =
        formulae ? sdm_parcel_launch_general_perm(ctx, call, formulae, coal->n_live, dv)
                 : sdm_parcel_launch_default_perm(ctx, call, coal->n_live, dv);
    if (launched != SDM_OK) return launched;
    a.at0 = step * n_parcel;
    const int collided = with_breakup ? COAL_DISPATCH(launch_coal, true, ctx, grid, lds, kc, A, a)
                                      : COAL_DISPATCH(launch_coal, false, ctx, grid, lds, kc, A, a);
    if (collided != SDM_OK) return collided;
  }
  return SDM_OK;
}

extern "C" int sdm_parcel_run_coal(
    sdm_ctx *ctx, const sdm_parcel_cfg *cfg, const sdm_step_cfg *coal_cfg, int64_t n_steps,
    int64_t n_parcel, int64_t n_sd, const int64_t *parcel_start, double *water_mass,
    int64_t *multiplicity, double *vdry, double *kappa, const double *f_org, double *v_cr,
    const sdm_parcel_state *state, const double *w_mid, const sdm_parcel_profile *profile,
    const double consts[34], const sdm_cond_formulae *formulae, const sdm_parcel_coal_state *coal,
    const sdm_parcel_coal_profile *coal_profile, int fresh_idx) {
  ARG_TRY(ctx && coal_cfg && coal);
  ARG_TRY(!coal_cfg->enable_breakup);  // (served by sdm_parcel_run_collision)
  return parcel_run_collision("sdm_parcel_run_coal", ctx, cfg, coal_cfg, n_steps, n_parcel, n_sd,
                              parcel_start, water_mass, multiplicity, vdry, kappa, f_org, v_cr,
                              state, w_mid, profile, consts, formulae, coal, coal_profile,
                              fresh_idx, nullptr, nullptr);
}

extern "C" int sdm_parcel_run_collision(
    sdm_ctx *ctx, const sdm_parcel_cfg *cfg, const sdm_step_cfg *coal_cfg, int64_t n_steps,
    int64_t n_parcel, int64_t n_sd, const int64_t *parcel_start, double *water_mass,
    int64_t *multiplicity, double *vdry, double *kappa, const double *f_org, double *v_cr,
    const sdm_parcel_state *state, const double *w_mid, const sdm_parcel_profile *profile,
    const double consts[34], const sdm_cond_formulae *formulae, const sdm_parcel_coal_state *coal,
    const sdm_parcel_coal_profile *coal_profile, int fresh_idx,
    const sdm_parcel_breakup_state *breakup, const sdm_parcel_breakup_profile *breakup_profile) {
  ARG_TRY(ctx && coal_cfg && coal);
  return parcel_run_collision("sdm_parcel_run_collision", ctx, cfg, coal_cfg, n_steps, n_parcel,
                              n_sd, parcel_start, water_mass, multiplicity, vdry, kappa, f_org,
                              v_cr, state, w_mid, profile, consts, formulae, coal, coal_profile,
                              fresh_idx, breakup, breakup_profile);
}
