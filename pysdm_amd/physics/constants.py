"""SI unit multipliers and the physical constants the collision path uses.

Values as in the reference's catalogue (PySDM/physics/constants.py:32-70,
PySDM/physics/constants_defaults.py:190,359-366,667), expressed in SI base units.
"""
import math
import os
import time
from types import SimpleNamespace


def _make_si():
    prefixes = {"n": 1e-9, "u": 1e-6, "m": 1e-3, "c": 1e-2, "d": 1e-1, "": 1.0, "h": 1e2,
                "k": 1e3}
    long_prefixes = {"nano": 1e-9, "micro": 1e-6, "milli": 1e-3, "centi": 1e-2, "deci": 1e-1,
                     "": 1.0, "hecto": 1e2, "kilo": 1e3}
    short_units = {"m": 1.0, "g": 1e-3, "s": 1.0, "J": 1.0, "K": 1.0, "Pa": 1.0, "l": 1e-3,
                   "N": 1.0, "W": 1.0, "Hz": 1.0, "mol": 1.0}
    long_units = {"metre": 1.0, "meter": 1.0, "gram": 1e-3, "second": 1.0, "joule": 1.0,
                  "kelvin": 1.0, "pascal": 1.0, "litre": 1e-3, "liter": 1e-3, "newton": 1.0,
                  "watt": 1.0, "hertz": 1.0, "mole": 1.0}
    table = {"dimensionless": 1.0, "min": 60.0, "minute": 60.0, "minutes": 60.0,
             "h": 3600.0, "hour": 3600.0, "hours": 3600.0, "day": 86400.0}
    for p_name, p_val in prefixes.items():
        for u_name, u_val in short_units.items():
            table.setdefault(p_name + u_name, p_val * u_val)
    for p_name, p_val in long_prefixes.items():
        for u_name, u_val in long_units.items():
            table[p_name + u_name] = p_val * u_val
            table[p_name + u_name + "s"] = p_val * u_val
    return SimpleNamespace(**table)


si = _make_si()

PI = math.pi
PI_4_3 = PI * 4 / 3
ONE_THIRD = 1 / 3
TWO_THIRDS = 2 / 3
ONE_AND_A_HALF = 3 / 2
CM = 1 * si.cm

rho_w = 1 * si.kilograms / si.litres
sgm_w = 0.072 * si.joule / si.metre**2

STRAUB_E_D1 = 0.04 * si.cm
STRAUB_MU2 = 0.095 * si.cm
VEDDER_1987_b = 89 / 880
VEDDER_1987_A = 993 / 880 / 3 / VEDDER_1987_b

# PySDM/physics/constants.py:50-54
default_random_seed = 44 if "CI" in os.environ else time.time_ns()

# Rogers & Yau terminal velocity (PySDM/physics/constants_defaults.py:625-635)
ROGERS_YAU_TERM_VEL_SMALL_K = 1.19e6 / si.cm / si.s
ROGERS_YAU_TERM_VEL_MEDIUM_K = 8e3 / si.s
ROGERS_YAU_TERM_VEL_LARGE_K = 2.01e3 * si.cm**0.5 / si.s
ROGERS_YAU_TERM_VEL_SMALL_R_LIMIT = 35 * si.um
ROGERS_YAU_TERM_VEL_MEDIUM_R_LIMIT = 600 * si.um

# condensation path (pysdm_amd/condensation.py): the values PySDM/physics/constants_defaults.py
# computes (Rv = R_str / Mv, Rd = R_str / Md, eps = Mv / Md, l_tri, Rd_over_c_pd = Rd / c_pd, the
# Flatau-Walko-Cotton coefficients in Pa, ...), written as the doubles it arrives at
Rv = 461.523055858115
Rd = 287.0421396862956
c_pd = 1005.0
c_pv = 1850.0
c_pw = 4218.0
l_tri = 2500711.849262262
T_tri = 273.16
T0 = 273.15
p1000 = 100000.0
g_std = 9.80665
eps = 0.6219453958862249
D0 = 2.26e-05
K0 = 0.024
MAC = 1.0
HAC = 1.0
Rd_over_c_pd = 0.28561406933959765
THREE = 3
FWC_C0 = 611.583699
FWC_C1 = 44.460689599999995
FWC_C2 = 1.43177157
FWC_C3 = 0.026422432099999997
FWC_C4 = 0.000299291081
FWC_C5 = 2.03154182e-06
FWC_C6 = 7.02620698e-09
FWC_C7 = 3.7953431e-12
FWC_C8 = -3.2158239300000003e-14
ZOGRAFOS_1987_COEFF_T3 = 2.5914e-15
ZOGRAFOS_1987_COEFF_T2 = -1.4346e-11
ZOGRAFOS_1987_COEFF_T1 = 5.0523e-08
ZOGRAFOS_1987_COEFF_T0 = 4.113e-06

# freezing path (pysdm_amd/freezing.py): ice density, the Flatau-Walko-Cotton coefficients of the
# saturation vapour pressure over ice (Flatau et al. 1992, in Pa), ABIFM (Knopf & Alpert 2013: M
# and C depend on the ice nucleus and have no default), the homogeneous rates of Koop et al. 2000,
# its correction by Spichtinger et al. 2023 and Koop & Murray 2016 (tab. VII); the constant rates
# J_HET / J_HOM have no default either (PySDM/physics/constants_defaults.py:139-155,188,312-356,
# written as the doubles it arrives at)
rho_i = 916.8
FWC_I0 = 609.868993
FWC_I1 = 49.9320233
FWC_I2 = 1.84672631
FWC_I3 = 0.0402737184
FWC_I4 = 0.000565392987
FWC_I5 = 5.216939329999999e-06
FWC_I6 = 3.0783958300000004e-08
FWC_I7 = 1.0578516000000001e-10
FWC_I8 = 1.61444444e-13
J_HET = math.nan
J_HOM = math.nan
ABIFM_M = math.inf
ABIFM_C = math.inf
ABIFM_UNIT = 10000.0
KOOP_2000_C1 = -906.7
KOOP_2000_C2 = 8502
KOOP_2000_C3 = -26924
KOOP_2000_C4 = 29180
KOOP_CORR = -1.522
KOOP_UNIT = 999999.9999999999
KOOP_MIN_DA_W_ICE = 0.26
KOOP_MAX_DA_W_ICE = 0.34
KOOP_MURRAY_C0 = -3020.684
KOOP_MURRAY_C1 = -425.921
KOOP_MURRAY_C2 = -25.9779
KOOP_MURRAY_C3 = -0.868451
KOOP_MURRAY_C4 = -0.0166203
KOOP_MURRAY_C5 = -0.000171736
KOOP_MURRAY_C6 = -7.46953e-07

# vapour deposition on ice (pysdm_amd/deposition.py): molar mass of water, the latent heat of
# sublimation of Murphy & Koop 2005 (eq. 5, J / mol), the mean free path of vapour in air at
# T_STP / p_STP and the Cunningham factor of the transition-regime correction (Pruppacher & Klett
# 2010), mass and heat accommodation coefficients of ice, the capacity of columnar crystals of
# Spichtinger et al. 2023 (eq. A11-A12) (PySDM/physics/constants_defaults.py:87-107,227,277-290,
# 532-538, written as the doubles it arrives at)
Mv = 0.018015270337240392
MK05_SUB_C1 = 46782.5
MK05_SUB_C2 = 35.8925
MK05_SUB_C3 = 0.07414
MK05_SUB_C4 = 541.5
MK05_SUB_C5 = 123.75
lmbd_w_0 = 6.6e-08
T_STP = 288.15
p_STP = 101325.0
C_cunn = 0.7
MAC_ice = 0.5
HAC_ice = 1.0
capacity_columnar_ice_A1 = 0.015755
capacity_columnar_ice_B1 = 0.3
capacity_columnar_ice_A2 = 0.33565
capacity_columnar_ice_B2 = 0.43

# aqueous chemistry (PySDM/physics/constants_defaults.py:31,87,293-296,772 and constants.py:67-68,
# written as the doubles it arrives at)
R_str = 8.31446261815324
Md = 0.028966000000000002
ROOM_TEMP = 298.15
M = 1000.0
K_H2O = 1e-08
H_u = M / p_STP
dT_u = 1.0
pH_w = 7

# condensation with non-default formulae (pysdm_amd/condensation.py, include/
# sdm_condensation_formulae.h): the organic-film surface tensions (Ovadnevaite et al. 2017, Ruehl
# et al. 2016: the film's parameters depend on the organic species and have no default), the
# saturation vapour pressures of August-Roche-Magnus, Bolton 1980, Lowe 1977, Murphy & Koop 2005
# and Wexler 1976, the latent heat, diffusivity and conductivity of Lowe et al. 2019, the
# diffusivity exponent of Tracy, Welch & Porter, the fits of Grabowski et al. 2011, the Pruppacher &
# Klett 2005 jump length and the ventilation coefficients of Froessling 1938 and Pruppacher &
# Rasmussen 1979 (PySDM/physics/constants_defaults.py:90,111-117,158-171,207-236,251-275,298-305,
# 557-601,638-673,770, written as the doubles it arrives at)
ONE_HALF = 1 / 2
N_A = 6.02214076e+23
water_molar_volume = 1.8015270337240393e-05
sgm_org = math.nan
delta_min = math.nan
RUEHL_nu_org = math.nan
RUEHL_A0 = math.nan
RUEHL_C0 = math.nan
RUEHL_m_sigma = math.nan
RUEHL_sgm_min = math.nan
ARM_C1 = 610.9399999999999
ARM_C2 = 17.625
ARM_C3 = 243.04
B80W_G0 = 611.2
B80W_G1 = 17.67
B80W_G2 = 243.5
L77W_A0 = 610.7799961000001
L77W_A1 = 44.36518521
L77W_A2 = 1.4289458050000001
L77W_A3 = 0.026506484709999997
L77W_A4 = 0.0003031240396
L77W_A5 = 2.034080948e-06
L77W_A6 = 6.136820928999999e-09
MK05_LIQ_C1 = 1.0
MK05_LIQ_C2 = 54.842763
MK05_LIQ_C3 = 6763.22
MK05_LIQ_C4 = 4.21
MK05_LIQ_C5 = 1.0
MK05_LIQ_C6 = 0.000367
MK05_LIQ_C7 = 0.0415
MK05_LIQ_C8 = 218.8
MK05_LIQ_C9 = 53.878
MK05_LIQ_C10 = 1331.22
MK05_LIQ_C11 = 9.44523
MK05_LIQ_C12 = 1.0
MK05_LIQ_C13 = 0.014025
W76W_G0 = -2991.2729
W76W_G1 = -6017.0128
W76W_G2 = 18.87643854
W76W_G3 = -0.028354721
W76W_G4 = 1.7838301e-05
W76W_G5 = -8.4150417e-10
W76W_G6 = 4.4412543e-13
W76W_G7 = 2.858487
W76W_G8 = 1.0
one_kelvin = 1.0
l_l19_a = 0.167
l_l19_b = 0.000365
d_l19_a = 2.11e-05
d_l19_b = 1.94
k_l19_a = 0.0042
k_l19_b = 1.0456
k_l19_c = 0.017
D_exp = 1.81
diffusion_thermics_D_G11_A = 1e-05
diffusion_thermics_D_G11_B = 0.015
diffusion_thermics_D_G11_C = -1.9
diffusion_thermics_K_G11_A = 1.5e-11
diffusion_thermics_K_G11_B = -4.8e-08
diffusion_thermics_K_G11_C = 0.0001
diffusion_thermics_K_G11_D = -0.00039
dv_pk05 = 0.0
FROESSLING_1938_A = 1
FROESSLING_1938_B = 0.276
PRUPPACHER_RASMUSSEN_1979_XTHRES = 1.4
PRUPPACHER_RASMUSSEN_1979_CONSTSMALL = 1.0
PRUPPACHER_RASMUSSEN_1979_COEFFSMALL = 0.108
PRUPPACHER_RASMUSSEN_1979_POWSMALL = 2.0
PRUPPACHER_RASMUSSEN_1979_CONSTBIG = 0.78
PRUPPACHER_RASMUSSEN_1979_COEFFBIG = 0.308


def namespace(overrides=None):
    """the numeric constants of this module as one namespace, optionally with overrides"""
    values = {name: value for name, value in globals().items()
              if not name.startswith("_") and isinstance(value, (int, float))
              and not isinstance(value, bool)}
    values.update(overrides or {})
    return SimpleNamespace(**values)
