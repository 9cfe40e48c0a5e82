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
  }
  if (d == 0) A.ctl[CTL_PAIRS] += W / 2;
  const double u = draw_at(A.s_rand, A.rng_inc, A.rng_aff, d);
  PairInfo R;
  R.have = false; R.off = 2; R.prob = 0; R.j = R.k = 0;
  if (d < (cfg.n_sd + 1) / 2) R = pair_prob_body<KERNEL, false>(cfg, A, d, W, 0.0, &L);
  double p = R.prob;
  if (p != 0) p /= (double)cfg.substeps;  // collision.py:279
  pair_update_body<false>(cfg, A, d, d < W / 2, p, u, 0.0, true, R.off, R.j, R.k, 2 * d + R.off,
                          true);
  PAIR_PROF_EXIT(1);
