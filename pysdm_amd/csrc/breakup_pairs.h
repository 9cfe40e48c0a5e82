// breakup_pairs.h -- what the kernels that resolve a COLLIDING pair with breakup share: the
// coalescence efficiency and the fragment mass of the pair (breakup_params).  fused.hip's
// resolve_collision and k_parcel_coal's breakup branch (parcel_coal.hip) evaluate a pair through
// this function, so that the two agree to the bit by construction.  The text is the one fused.hip
// held before the parcel with breakup needed it in a second translation unit.
#ifndef SDM_BREAKUP_PAIRS_H
#define SDM_BREAKUP_PAIRS_H
#include "collision_pairs.h"

// Ec (coalescence efficiency) and fragment mass of one pair from the members' masses -- only
// evaluated for pairs that actually collide (they are pure functions of the pair's state before
// the update, so evaluating them lazily gives the values the reference computes for all pairs)
__device__ __forceinline__ void breakup_params(const sdm_step_cfg &cfg, const FusedArgs &A,
                                               const SD &sj, const SD &sk, double u_b,
                                               double &ec, double &fm) {
  const double mj = sj.m, mk = sk.m;
  const double vj = volume_of_mass(mj, cfg.rho_w), vk = volume_of_mass(mk, cfg.rho_w);
  const double rj = sj.r, rk = sk.r, uj = sj.u, uk = sk.u;
    switch (cfg.ec) {
      case SDM_EC_CONST: ec = cfg.ec_param[0]; break;
      case SDM_EC_BERRY1967: {
        const double e = linear_collection_efficiency(cfg.berry_params, rj, rk, cfg.berry_unit);
        ec = signed_sq(e);
        break;
      }
      case SDM_EC_LOWLIST1982: {  // coalescence_efficiencies/lowlist1982.py:37-103 (mass-based)
        const double PI = 3.14159265358979323846;
        const double ds = (rj < rk ? rj : rk) * 2, dl = (rj > rk ? rj : rk) * 2;
        double Sc = signed_pow(mj + mk, 2.0 / 3.0);
        Sc *= cfg.ec_param[1];  // PI * sgm_w * (6/PI)**(2/3), one host-side constant
        double St = ds * ds;
        St += dl * dl;
        St *= PI * cfg.sgm_w;
        const double dS = St - Sc;
        const double tmp = mj + mk;
        double tmp2 = fabs(uj - uk);
        tmp2 = tmp2 * tmp2;
        double CKE = mj * mk;
        if (tmp != 0.0) CKE /= tmp;
        CKE *= tmp2;
        CKE *= cfg.rho_w / 2;
        const double Et = CKE + dS;
        double e = signed_sq(Et);
        e *= -1.0 * 2.61e6 * cfg.sgm_w;
        e /= Sc;
        double o = ds / dl;
        o += 1.0;
        o = signed_pow(o, -2.0);
        o *= 0.778;
        o *= sdm_exp(e);
        ec = dl < 0.4e-3 ? 1.0 : o;
        break;
      }
      default: {  // coalescence_efficiencies/straub2010.py:27-50
        double tmp = vj + vk;
        double Sc = tmp * (6 / 3.14159265358979323846);
        tmp *= 2;
        double tmp2 = fabs(uj - uk);
        tmp2 = tmp2 * tmp2;
        double We = vj * vk;
        if (tmp != 0.0) We /= tmp;
        We *= tmp2;
        We *= cfg.rho_w;
        Sc = signed_pow(Sc, 2.0 / 3.0);
        Sc *= 3.14159265358979323846 * cfg.sgm_w;
        if (Sc != 0.0) We /= Sc;
        We *= -1.15;
        ec = sdm_exp(We);
      }
    }
    switch (cfg.frag) {
      case SDM_FRAG_ALWAYS_N: fm = (mj + mk) / cfg.frag_param[0]; break;
      case SDM_FRAG_EXPONENTIAL: {
        const double a = 1 - u_b;
        double fv = -cfg.frag_param[0] * sdm_log(PYMAX(a, 1e-5)), nf;
        fragmentation_limiters(nf, fv, cfg.frag_vmin, cfg.frag_nfmax, vj + vk);
        fm = cfg.rho_w * fv;
        break;
      }
      case SDM_FRAG_GAUSSIAN: {  // fragmentation_methods.py:477-485
        double fv = cfg.frag_param[0] + cfg.frag_param[1] *
                    erfinv_approx(u_b, cfg.straub_consts[3], cfg.straub_consts[4]), nf;
        fragmentation_limiters(nf, fv, cfg.frag_vmin, cfg.frag_nfmax, vj + vk);
        fm = cfg.rho_w * fv;
        break;
      }
      case SDM_FRAG_FEINGOLD1988: {  // :487-499, physics/fragmentation_function/feingold1988.py
        const double a = 1 - u_b * cfg.frag_param[0] / (vj + vk);
        double fv = -cfg.frag_param[0] * sdm_log(PYMAX(a, cfg.frag_param[1])), nf;
        fragmentation_limiters(nf, fv, cfg.frag_vmin, cfg.frag_nfmax, vj + vk);
        fm = cfg.rho_w * fv;
        break;
      }
      case SDM_FRAG_SLAMS: {  // :95-134
        double p = 0.0, nf = 1;
        for (int k = 0; k < 22; ++k) {
          p += 0.91 * sdm_pow((double)(k + 2), -1.56);
          if (u_b < p) { nf = k + 2; break; }
        }
        double fv = (vj + vk) / nf;
        fragmentation_limiters(nf, fv, cfg.frag_vmin, cfg.frag_nfmax, vj + vk);
        fm = cfg.rho_w * fv;
        break;
      }
      case SDM_FRAG_CONSTANT_MASS: fm = cfg.frag_param[0]; break;  // constant_mass.py:11-14
      case SDM_FRAG_LOWLIST1982: {  // breakup_fragmentations/lowlist82.py:37-103 (volume-based)
        const double PI = 3.14159265358979323846;
        const double x_plus_y = vj + vk;
        const double ds = (rj < rk ? rj : rk) * 2, dl = (rj > rk ? rj : rk) * 2;
        double dcoal = x_plus_y / (PI / 6);
        dcoal = signed_pow(dcoal, 1.0 / 3.0);
        double Sc = signed_pow(x_plus_y, 2.0 / 3.0);
        Sc *= cfg.frag_param[0];  // PI * sgm_w * (6/PI)**(2/3), one host-side constant
        double St = ds * ds;
        St += dl * dl;
        St *= PI * cfg.sgm_w;
        double tmp2 = fabs(uj - uk);
        tmp2 = tmp2 * tmp2;
        double CKE = vj * vk;
        if (x_plus_y != 0.0) CKE /= x_plus_y;
        CKE *= tmp2;
        CKE *= cfg.rho_w / 2;
        double We = CKE, W2 = CKE;
        if (Sc != 0.0) We /= Sc;
        if (St != 0.0) W2 /= St;
        const double K[4] = {cfg.straub_consts[0], cfg.straub_consts[5], cfg.straub_consts[3],
                             cfg.straub_consts[4]};
        double rand = u_b, Rf = 0.0, Rs = 0.0, Rd = 0.0, nf;
        double fv = ll82_fragment_volume(CKE, We, W2, St, ds, dl, dcoal, &rand, &Rf, &Rs, &Rd,
                                         1e-8, K);
        fragmentation_limiters(nf, fv, cfg.frag_vmin, cfg.frag_nfmax, x_plus_y);
        fm = cfg.rho_w * fv;
        break;
      }
      default: {  // breakup_fragmentations/straub2010.py:42-101
        const double v_max = vj > vk ? vj : vk;
        const double x_plus_y = vj + vk;
        const double ds = (rj < rk ? rj : rk) * 2;
        double tmp = vj + vk;
        double Sc = signed_pow(tmp, 2.0 / 3.0);
        Sc *= cfg.frag_param[1];  // PI * sgm_w * (6/PI)**(2/3), one host-side constant
        double tmp2 = fabs(uj - uk);
        tmp2 = tmp2 * tmp2;
        double CKE = vj * vk;
        if (tmp != 0.0) CKE /= tmp;
        CKE *= tmp2;
        CKE *= cfg.rho_w / 2;
        double We = CKE;
        if (Sc != 0.0) We /= Sc;
        double CW = We;
        CW *= CKE;
        CW /= 1e-6;  // si.uJ
        double gam = rj > rk ? rj : rk;
        const double rmin = rj < rk ? rj : rk;
        if (rmin != 0.0) gam /= rmin;
        StraubTmp T = {0, 0, 0, 0, 0, 0};
        double fv = straub_fragment_volume(CW, gam, ds, v_max, u_b, cfg.straub_consts, T), nf;
        fragmentation_limiters(nf, fv, cfg.frag_vmin, cfg.frag_nfmax, x_plus_y);
        fm = cfg.rho_w * fv;
      }
    }
}

#endif  // SDM_BREAKUP_PAIRS_H
