/* TEST INFRASTRUCTURE, NOT PRODUCT CODE: pysdm_amd/csrc/pair_tag.h compiled for the host, array by
 * array (tests/test_pair_tag_model.py, scripts/pair_tag_share.py).  The exported functions loop
 * over the header's own and over the model of the kernel's decision below. */
#include "../../pysdm_amd/csrc/pair_tag.h"

#define API __attribute__((visibility("default")))

API int pt_shift(void) { return PAIR_TAG_SHIFT; }
API int pt_bits(void) { return PAIR_TAG_BITS; }

API double pt_m_base(double m_max) { return pair_tag_m_base(pair_tag_f64_to_bits(m_max)); }

API void pt_encode(const int64_t *n, const double *m, int64_t count, int64_t n_ref, double m_base,
                   uint32_t *tag) {
  for (int64_t i = 0; i < count; ++i) tag[i] = pair_tag_encode(n[i], m[i], n_ref, m_base);
}

/* upper bounds of the classes; -1 / -1.0 where the class is "unknown" */
API void pt_bounds(const uint32_t *tag, int64_t count, int64_t n_ref, double m_base, int64_t *n_ub,
                   double *m_ub) {
  for (int64_t i = 0; i < count; ++i) {
    n_ub[i] = pair_tag_nc(tag[i]) ? pair_tag_n_ub(tag[i], n_ref) : -1;
    m_ub[i] = pair_tag_mc(tag[i]) ? pair_tag_m_ub(tag[i], m_base) : -1.0;
  }
}

API void pt_order(const uint32_t *tag_j, const uint32_t *tag_k, int64_t count, int8_t *order) {
  for (int64_t i = 0; i < count; ++i) order[i] = (int8_t)pair_tag_order(tag_j[i], tag_k[i]);
}

/* What the pair kernel does with the header's two decisions (fused.hip, pair_prob_body): the bound
 * of the Golovin probability from the bounds of the tags, operation by operation as
 * pair_prob_value<SDM_KERNEL_GOLOVIN> has it, and the whole decision for a pair of tags and a draw:
 * 1 = skipped (order in *swap), 0 = gather */
static double golovin_bound(int64_t n, double mj, double mk, double b, double rho_w, double norm,
                            int64_t substeps) {
  const double vj = mj / rho_w, vk = mk / rho_w;
  const double K = (vj + vk) * b;
  double prob = (double)n;
  prob *= K;
  prob *= norm;
  if (prob != 0) prob /= (double)substeps;
  return prob;
}
static int pair_tag_decide(uint32_t tag_j, uint32_t tag_k, double u, int64_t n_ref, double m_base,
                           double b, double rho_w, double norm, int64_t substeps, int *swap) {
  const int order = pair_tag_order(tag_j, tag_k);
  if (order < 0) return 0;
  *swap = order;
  if (order) {
    const uint32_t t = tag_j; tag_j = tag_k; tag_k = t;
  }
  if (pair_tag_mc(tag_j) == 0 || pair_tag_mc(tag_k) == 0) return 0;
  const double p_ub = golovin_bound(pair_tag_n_ub(tag_j, n_ref), pair_tag_m_ub(tag_j, m_base),
                                    pair_tag_m_ub(tag_k, m_base), b, rho_w, norm, substeps);
  return pair_tag_no_collision(p_ub, u) ? 1 : 0;
}

/* skipped[i] = 1: the pair is decided from its tags (swap[i] = its order); 0: it gathers */
API void pt_decide(const uint32_t *tag_j, const uint32_t *tag_k, const double *u, int64_t count,
                   int64_t n_ref, double m_base, double b, double rho_w, double norm,
                   int64_t substeps, uint8_t *skipped, uint8_t *swap) {
  for (int64_t i = 0; i < count; ++i) {
    int s = 0;
    skipped[i] = (uint8_t)pair_tag_decide(tag_j[i], tag_k[i], u[i], n_ref, m_base, b, rho_w, norm,
                                          substeps, &s);
    swap[i] = (uint8_t)s;
  }
}
