// The body of k_pair_all_sort<KERNEL> and of its sibling k_pair_all_sort_closed<KERNEL>
// (fused.hip), included into both: the kernel the Gunn-Kinzer table is launched with has this text
// inside itself, as before the fall-velocity laws came, and compiles to the instructions it
// compiled to then.  (As a function called by both it cost that kernel 23 to 47 instructions and
// two SGPRs kept in VGPR lanes.)  In scope: cfg, A, X, KERNEL.
  extern __shared__ __attribute__((aligned(16))) char smem[];
  PAIR_PROF_ENTRY();
  if ((int)blockIdx.x < X.n_tiles) {
    const int64_t length = *X.p_length;
    bin_sort_body<true>(smem, X.events, X.toff, X.jarr, X.loc, X.n_bins, nullptr, nullptr, 1,
                        length, length, X.s_off, A.rng_inc, A.rng_tab, nullptr, A.rng_aff);
    PAIR_PROF_EXIT(0);
    return;
  }
  const int64_t W = A.ctl[CTL_WORK];
  // (two pair workgroups per tile: block numbers 8 apart, pair_block)
  const unsigned lb = pair_block(A, blockIdx.x - X.n_tiles, gridDim.x - X.n_tiles, BIN_THREADS);
  const int64_t d = (int64_t)lb * BIN_THREADS + threadIdx.x;
  // The first look-up of a walk: for the 63 % of the positions whose own event is their last it
  // is an S word whose place lies in the position's own tile (shuffle_build.h: place = tile_first +
  // at) - 4096 random 4-byte reads per tile into one 16-KB segment of ssucc.  The workgroup loads
  // its tile's segment coalesced (16 bytes per lane, in flight together with the slot's words of
  // `first`) into the dynamic LDS that only the sorting workgroups used, and the walks take that
  // look-up from there.  Successor words from 4096-event tiles only; the tables are whole tiles.
  WalkSeg L;
  L.seg = nullptr; L.seg_first = L.seg_len = L.n0 = L.n1 = 0;
  const int64_t my_tile = 2 * (int64_t)lb * BIN_THREADS / EV_TILE;
  // {both counts of a tagged step, waves that have added theirs} (the end of this text), zero
  // before the first barrier
  __shared__ unsigned tag_cnt[2];
  const bool tag_count = PAIR_BODY_TAGS && PAIR_TAG_COUNT && (A.narrow & NARROW_TAG_OUT) &&
                         (A.narrow & NARROW_TAG_IN);  // uniform
  if (tag_count && threadIdx.x < 2) tag_cnt[threadIdx.x] = 0;
#ifdef WALK_NO_SEG  // (tuning builds: every look-up from the tables)
  if (false) {
#else
  if (A.walk_tile == EV_TILE && A.rec_fmt == SDM_REC_CHAIN && my_tile < A.walk_tiles) {  // uniform
#endif
    const uint2 w = *(const uint2 *)((const uint32_t *)A.rec + 2 * d);
    const sort_v4u *from = (const sort_v4u *)((const uint32_t *)A.ovf_next + my_tile * EV_TILE);
    for (int q = threadIdx.x; q < EV_TILE / 4; q += BIN_THREADS) ((sort_v4u *)smem)[q] = from[q];
    // (LDS only, as in k_bin_build2; the stores above have waited for their loads)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    L.seg = (const uint32_t *)smem;
    L.seg_first = (uint32_t)(my_tile * EV_TILE);
    L.seg_len = EV_TILE;
    L.n0 = w.x;
    L.n1 = w.y;
  } else if (tag_count) {
    __syncthreads();
  }
  if (d == 0) A.ctl[CTL_PAIRS] += W / 2;
  const double u = draw_at(A.s_rand, A.rng_inc, A.rng_aff, d);
  PairInfo R;
  R.have = false; R.off = 2; R.prob = 0; R.j = R.k = 0;
  // PAIR_BODY_TAGS (set by the including kernel; true in k_pair_all_sort<Golovin> alone): tags
  // beside the ids (pair_tag.h).  Everywhere else the lines below are what they were
  constexpr bool TAGGED = PAIR_BODY_TAGS;
  PairTags T;
  T.u = u; T.tj = T.tk = 0; T.skipped = false; T.mj = T.mk = 0.0;
  if (d < (cfg.n_sd + 1) / 2)
    R = pair_prob_body<KERNEL, false, TAGGED>(cfg, A, d, W, 0.0, &L, TAGGED ? &T : nullptr);
  double p = R.prob;
  if (p != 0) p /= (double)cfg.substeps;  // collision.py:279
  const bool tag_out = TAGGED && (A.narrow & NARROW_TAG_OUT);
  const int died = pair_update_body<false>(cfg, A, d, d < W / 2, p, u, 0.0, true, R.off, R.j, R.k,
                                           2 * d + R.off, !tag_out);
  if (tag_out) {
    if (R.have) {
      // the slot's two words (i = 2d on this route): a skipped pair keeps the tags it came with,
      // a gathered one gets those of its state as the update left it; a dead member the bare flag
      uint32_t tj = T.tj, tk = T.tk;
      if (!T.skipped) {
        int64_t nj = R.nj, nk = R.nk;
        double mj = T.mj, mk = T.mk;
        if (ceil(p - u) != 0) {  // collided: this thread's own writes, read back
          const SD sj = sd_load(cfg, A, R.j, false), sk = sd_load(cfg, A, R.k, false);
          nj = sj.n; mj = sj.m;
          nk = sk.n; mk = sk.m;
        }
        const int64_t n_ref = A.slots[TAG_N_REF];
        const double m_base = pair_tag_m_base(A.slots[TAG_M_MAX]);
        tj = pair_tag_encode(nj, mj, n_ref, m_base);
        tk = pair_tag_encode(nk, mk, n_ref, m_base);
      }
      const uint32_t wj = (died & 1) ? (uint32_t)cfg.n_sd : (uint32_t)R.j | (tj << PAIR_TAG_SHIFT);
      const uint32_t wk = (died & 2) ? (uint32_t)cfg.n_sd : (uint32_t)R.k | (tk << PAIR_TAG_SHIFT);
      *(int2 *)((int32_t *)A.idx + 2 * d) = make_int2((int32_t)wj, (int32_t)wk);
    }
    if (tag_count) {
      // a tagged step's pairs by what became of them: one add per count and workgroup, made by
      // the wave that arrives last - no barrier, a wave that is done leaves.  Both counts in one
      // LDS word, at most BIN_THREADS = 2^10 each.  (The counting costs 0.5 us of the step with or
      // without a barrier here: profiles/README.md, round 10; -DPAIR_TAG_COUNT=0 leaves it out)
      const unsigned skipped = __popcll(__ballot(R.have && T.skipped));
      const unsigned gathered = __popcll(__ballot(R.have && !T.skipped));
      if (lane_id() == 0) {
        atomicAdd(&tag_cnt[0], skipped | (gathered << 16));
        if (atomicAdd(&tag_cnt[1], 1u) == BIN_THREADS / SDM_WAVE - 1) {
          const unsigned both = atomicAdd(&tag_cnt[0], 0u);  // (after every wave's add: LDS keeps a wave's order)
          int64_t *slot = &A.slots[(blockIdx.x & (SDM_CNT_SLOTS - 1)) * SDM_CNT_STRIDE + SLOT_TAG_SKIPPED];
          if (both & 0xffffu) atomicAdd((unsigned long long *)&slot[0], (unsigned long long)(both & 0xffffu));
          if (both >> 16) atomicAdd((unsigned long long *)&slot[1], (unsigned long long)(both >> 16));
        }
      }
    }
  }
  PAIR_PROF_EXIT(1);
