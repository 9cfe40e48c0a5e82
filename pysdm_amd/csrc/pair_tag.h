// pair_tag.h -- nine bits of bounds on a super-droplet's state, carried beside its id in the 32-bit
// permutation word between the steps of one call (fused.hip: k_pair_all_sort<Golovin> writes them,
// the next build hands them to the walks' ends verbatim).  Plain functions for host and device, no
// HIP types: tests/test_pair_tag_model.py and scripts/pair_tag_share.py compile this file with the
// host compiler.
//
// word = id | tag << PAIR_TAG_SHIFT;  tag = nc | ex << 4 | mc << 5, all zero = nothing known
//   nc (4 bits): octave of the multiplicity below n_ref.  c in 1..15: n_ref / 2^c < n <= n_ref /
//      2^(c-1) - for integers (n_ref >> c) < n <= (n_ref >> (c-1)); the intervals are disjoint, so
//      a higher class is a strictly smaller multiplicity.  0: n <= 0, n > n_ref, n <= n_ref >> 15
//   ex (1 bit): n << (c-1) == n_ref, the multiplicity IS n_ref >> (c-1) and the shift lost nothing
//   mc (4 bits): 1: 0 < m <= m_base; c in 2..15: m_base * 4^(c-2) < m <= m_base * 4^(c-1); 0: not
//      finite, <= 0 or above the top class.  m_base is a power of two: every edge is exact
// Any n_ref and m_base give sound tags; the largest multiplicity and 2^-16 of the power of two above
// the largest mass at the start of the call make them sharp.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PAIR_TAG_FN __host__ __device__ __forceinline__
#else
#if !defined(__cplusplus)
#include <stdbool.h>
#endif
#define PAIR_TAG_FN static inline
#endif

#define PAIR_TAG_BITS 9
#define PAIR_TAG_SHIFT 21  // ids and the `n_sd` flag below 2^21: 30 payload bits of a successor word
#define PAIR_TAG_ID_MASK ((1u << PAIR_TAG_SHIFT) - 1)

PAIR_TAG_FN double pair_tag_bits_to_f64(int64_t b) {
  union { int64_t i; double d; } v;
  v.i = b;
  return v.d;
}
PAIR_TAG_FN int64_t pair_tag_f64_to_bits(double d) {
  union { int64_t i; double d; } v;
  v.d = d;
  return v.i;
}

// m_base from the bit pattern of the largest (positive, finite) mass: the power of two at or above
// it, divided by 2^16.  0 - every mass class unknown - for anything else or where that underflows
PAIR_TAG_FN double pair_tag_m_base(int64_t m_max_bits) {
  if (m_max_bits <= 0) return 0.0;
  int64_t e = (m_max_bits >> 52) & 0x7ff;
  if (e == 0x7ff) return 0.0;
  if (m_max_bits & ((1ll << 52) - 1)) e += 1;
  e -= 16;
  if (e <= 0 || e >= 0x7ff) return 0.0;
  return pair_tag_bits_to_f64(e << 52);
}

PAIR_TAG_FN uint32_t pair_tag_nc(uint32_t tag) { return tag & 15u; }
PAIR_TAG_FN uint32_t pair_tag_ex(uint32_t tag) { return (tag >> 4) & 1u; }
PAIR_TAG_FN uint32_t pair_tag_mc(uint32_t tag) { return (tag >> 5) & 15u; }

// (no loops: the pair kernel encodes two tags per gathered pair)
PAIR_TAG_FN int pair_tag_bit_length(uint64_t x) { return x ? 64 - __builtin_clzll(x) : 0; }
PAIR_TAG_FN uint32_t pair_tag_encode(int64_t n, double m, int64_t n_ref, double m_base) {
  uint32_t tag = 0;
  if (n > 0 && n <= n_ref) {
    // n_ref >> d has n's bit length: the class is d where n is the larger of the two, else d + 1
    const int d = pair_tag_bit_length((uint64_t)n_ref) - pair_tag_bit_length((uint64_t)n);
    const int c = n > (n_ref >> d) ? d : d + 1;
    if (c <= 15) tag = (uint32_t)c | ((n << (c - 1)) == n_ref ? 16u : 0u);
  }
  const int64_t mb = pair_tag_f64_to_bits(m), bb = pair_tag_f64_to_bits(m_base);
  if (mb > 0 && mb < (0x7ffll << 52) && bb > 0) {  // positive and finite; m_base a power of two
    // t = ceil(log2(m / m_base)) from the exponent fields (a subnormal m: field 0, far below)
    const int64_t t = (mb >> 52) - (bb >> 52) + ((mb & ((1ll << 52) - 1)) ? 1 : 0);
    const int64_t c = t <= 0 ? 1 : 1 + (t + 1) / 2;  // the smallest c with 2 (c - 1) >= t
    if (c <= 15) tag |= (uint32_t)c << 5;
  }
  return tag;
}

// upper bounds the classes stand for (class != 0).  The multiplicity's is the same whether `ex` is
// set or not: an integer below the class's upper edge is at most its floor, and the exact value
// is that floor
PAIR_TAG_FN int64_t pair_tag_n_ub(uint32_t tag, int64_t n_ref) {
  return n_ref >> (pair_tag_nc(tag) - 1);
}
PAIR_TAG_FN double pair_tag_m_ub(uint32_t tag, double m_base) {
  return m_base * (double)(1ll << (2 * (pair_tag_mc(tag) - 1)));
}

// order within the pair (sort_within_pair_by_attr: swap = n_j < n_k) from the tags alone:
// 0 = j stays first, 1 = swap, -1 = not known
PAIR_TAG_FN int pair_tag_order(uint32_t tag_j, uint32_t tag_k) {
  const uint32_t cj = pair_tag_nc(tag_j), ck = pair_tag_nc(tag_k);
  if (cj == 0 || ck == 0) return -1;
  if (cj != ck) return cj > ck ? 1 : 0;
  return (pair_tag_ex(tag_j) & pair_tag_ex(tag_k)) ? 0 : -1;
}

// whether the bound of the probability, p_ub - evaluated like the probability itself from
// pair_tag_n_ub of the first member and pair_tag_m_ub of both, divided by the sub-steps - excludes
// a collision for the draw u: gamma = ceil(p - u) is then zero in the full computation too.  The
// factor keeps a difference in rounding or contraction between the two evaluations from mattering
PAIR_TAG_FN double pair_tag_guard(double p_ub) { return p_ub * (1.0 + 1.0 / 1073741824.0); }
PAIR_TAG_FN bool pair_tag_no_collision(double p_ub, double u) {
  const double d = pair_tag_guard(p_ub) - u;
  return d <= 0 && d > -1;
}
