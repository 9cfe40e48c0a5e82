"""Binding of include/sdm_hip.h generated from the header itself.

The header is the single description of the boundary; this module parses its prototypes once and
builds, for any shared library that implements them, a table of callables that
  * accept device arrays (torch tensors), host arrays (numpy) or ctypes objects for pointer
    parameters and Python numbers / sequences for scalar and fixed-size host-array parameters,
  * check on the host, before anything is launched, that every array is contiguous and of the
    element type the C parameter names (double <-> float64, int64_t <-> int64, uint8_t <-> bool /
    uint8) - a kernel must never see an operand it was not written for,
  * turn a non-zero return code into a RuntimeError carrying `sdm_last_error()`.
The product library is pysdm_amd/libsdm_hip.so (HIP kernels, device pointers).  The CPU oracle
(oracle/, test infrastructure) implements the same header for host pointers and is bound by the
same code.  There is no fallback between the two: a missing library or symbol is an ImportError.
"""
import ctypes
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sdm_hip.h")
# the condensation path has a header of its own (implemented by libsdm_hip.so, not by the oracle)
CONDENSATION_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sdm_condensation.h")
# and its formulae other than PySDM's defaults a further one (the `_f` symbols)
CONDENSATION_FORMULAE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include",
                                                 "sdm_condensation_formulae.h")
# and so has the freezing path
FREEZING_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sdm_freezing.h")
# and the vapour-deposition path
DEPOSITION_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sdm_deposition.h")
# and the aqueous-chemistry path
CHEMISTRY_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sdm_chemistry.h")
# and the seeding path
SEEDING_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sdm_seeding.h")
# and the relaxed-fall-velocity path
RELAXED_VELOCITY_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include",
                                            "sdm_relaxed_velocity.h")
# and the initialisation path (Koehler-equilibrium wet radii)
INITIALISATION_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include",
                                          "sdm_initialisation.h")
# and the adiabatic-parcel path (whole ascents of ensembles of parcels)
PARCEL_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sdm_parcel.h")
# and the parcel's diagnostics (moments and a size spectrum per step)
PARCEL_DIAG_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sdm_parcel_diag.h")
# and the parcel with aqueous chemistry (cloud processing of aerosol)
PARCEL_CHEM_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sdm_parcel_chem.h")
# and the ventilated parcel (Reynolds numbers inside the step loop)
PARCEL_VENT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sdm_parcel_vent.h")
# and the parcel with coalescence (condensation and collisions in one call)
PARCEL_COAL_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sdm_parcel_coal.h")
# and the parcel with collisional breakup (Collision and Breakup in the same call)
PARCEL_BREAKUP_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include",
                                          "sdm_parcel_breakup.h")
# and the mixed-phase parcel (freezing and vapour deposition on ice inside the step loop)
PARCEL_ICE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sdm_parcel_ice.h")
# SDM_HIP_LIB: another build of the same library (tuning variants); still no fallback
HIP_LIB_PATH = os.environ.get("SDM_HIP_LIB") or os.path.join(_HERE, "libsdm_hip.so")

c_i64, c_f64, c_int, c_ptr, c_u64 = (ctypes.c_int64, ctypes.c_double, ctypes.c_int,
                                     ctypes.c_void_p, ctypes.c_uint64)


VELOCITY_TERMINAL, VELOCITY_MOMENTUM = 0, 1  # SDM_VELOCITY_* of include/sdm_hip.h
# SDM_VELOCITY_LAW_*, by the names of pysdm_amd.terminal_velocity.LAWS
VELOCITY_LAWS = {"GunnKinzer1949": 0, "RogersYau": 1, "PowerSeries": 2}
VELOCITY_MAX_TERMS = 16


# ---- the structs of the fused entry points (layout checked against the header in tests/test_abi.py)
class StepCfg(ctypes.Structure):  # == sdm_step_cfg
    _fields_ = [
        ("n_sd", c_i64), ("n_cell", c_i64), ("n_attr", c_i64),
        ("dt", c_f64), ("dv", c_f64), ("dt_min", c_f64), ("dt_max", c_f64),
        ("adaptive", ctypes.c_int32), ("substeps", ctypes.c_int32),
        ("croupier_local", ctypes.c_int32), ("optimized_random", ctypes.c_int32),
        ("enable_breakup", ctypes.c_int32), ("handle_all_breakups", ctypes.c_int32),
        ("kernel", ctypes.c_int32), ("ec", ctypes.c_int32), ("frag", ctypes.c_int32),
        ("mass_attr", ctypes.c_int32),
        ("kernel_param", c_f64 * 2), ("ec_param", c_f64 * 2), ("eb_const", c_f64),
        ("frag_param", c_f64 * 2), ("frag_vmin", c_f64), ("frag_nfmax", c_f64),
        ("rho_w", c_f64), ("sgm_w", c_f64), ("straub_consts", c_f64 * 6),
        ("berry_params", c_f64 * 13), ("berry_unit", c_f64),
        ("kernel_berry_params", c_f64 * 13), ("kernel_berry_unit", c_f64),
        ("max_multiplicity", c_i64), ("rng_state_inc", c_u64 * 4),
        ("gk_table_len", c_i64), ("gk_factor", c_f64),
        ("velocity_source", ctypes.c_int32), ("momentum_attr", ctypes.c_int32),
        ("velocity_law", ctypes.c_int32), ("velocity_terms", ctypes.c_int32),
    ]


class StepState(ctypes.Structure):  # == sdm_step_state
    _fields_ = [
        ("idx", c_ptr), ("tmp_idx", c_ptr), ("multiplicity", c_ptr), ("attributes", c_ptr),
        ("cell_id", c_ptr), ("cell_idx", c_ptr), ("cell_start", c_ptr), ("dt_left", c_ptr),
        ("stats_dt_min", c_ptr), ("stats_n_substep", c_ptr), ("collision_rate", c_ptr),
        ("collision_rate_deficit", c_ptr), ("coalescence_rate", c_ptr), ("breakup_rate", c_ptr),
        ("breakup_rate_deficit", c_ptr), ("gk_a", c_ptr), ("gk_b", c_ptr), ("ctl", c_ptr),
        ("nm", c_ptr), ("known_valid", c_i64), ("rng_offset", c_u64),
        ("rng_offset_breakup", c_u64),
        ("cell_owned", c_ptr), ("exchange", c_ptr), ("exchange_user", c_ptr),
        ("xchg_cells", c_ptr), ("xchg_idx", c_ptr),
        ("shard_rank", ctypes.c_int32), ("shard_world", ctypes.c_int32),
        ("cell_id_by_id", c_ptr), ("velocity_params", c_ptr),
    ]


# sdm_exchange_fn
ExchangeFn = ctypes.CFUNCTYPE(c_int, c_ptr, c_int, c_ptr, c_i64)
XCHG_SUM_F64, XCHG_SUM_I64, XCHG_MIN_F64 = 1, 2, 3
COMM_ID_BYTES = 128


class StepResult(ctypes.Structure):  # == sdm_step_result
    _fields_ = [
        ("n_substeps", c_i64), ("n_pairs", c_i64), ("valid_n_sd", c_i64), ("idx_swapped", c_i64),
        ("rng_offset", c_u64), ("rng_offset_breakup", c_u64), ("ctl", c_i64 * 8),
    ]


class DispCfg(ctypes.Structure):  # == sdm_disp_cfg
    _fields_ = [
        ("n_sd", c_i64), ("n_dims", ctypes.c_int32), ("scheme", ctypes.c_int32),
        ("enable_sedimentation", ctypes.c_int32), ("n_substeps", ctypes.c_int32),
        ("grid", c_i64 * 3), ("strides", c_i64 * 3), ("dt_over_dz", c_f64), ("level", c_f64),
    ]


class DispState(ctypes.Structure):  # == sdm_disp_state
    _fields_ = [
        ("courant", c_ptr * 3), ("displacement", c_ptr), ("position_in_cell", c_ptr),
        ("cell_origin", c_ptr), ("cell_id", c_ptr), ("fall_velocity", c_ptr),
        ("water_mass", c_ptr), ("multiplicity", c_ptr), ("idx", c_ptr), ("ctl", c_ptr),
    ]


class DispShard(ctypes.Structure):  # == sdm_disp_shard
    _fields_ = [
        ("cell_owned", c_ptr), ("n_cell", c_i64), ("exchange", c_ptr), ("exchange_user", c_ptr),
        ("shard_rank", ctypes.c_int32), ("shard_world", ctypes.c_int32),
        ("xchg_counts", c_ptr), ("xchg_words", c_ptr), ("word_capacity", c_i64),
        ("cell_id_by_id", c_ptr), ("role", c_ptr), ("role_ready", ctypes.c_int32),
        ("multiplicity", c_ptr), ("attributes", c_ptr), ("n_attr", ctypes.c_int32),
        ("n_moved", c_i64), ("n_left", c_i64), ("n_arrived", c_i64), ("n_words", c_i64),
        ("n_removed", c_i64),
    ]


class FreezingCfg(ctypes.Structure):  # == sdm_freezing_cfg (include/sdm_freezing.h)
    _fields_ = [
        ("singular", ctypes.c_int32), ("immersion_freezing", ctypes.c_int32),
        ("homogeneous_freezing", ctypes.c_int32), ("thaw", ctypes.c_int32),
        ("j_het", ctypes.c_int32), ("j_hom", ctypes.c_int32), ("rates", ctypes.c_int32),
        ("reserved", ctypes.c_int32), ("timestep", c_f64), ("rng_state_inc", c_u64 * 4),
    ]


class DepositionCfg(ctypes.Structure):  # == sdm_deposition_cfg (include/sdm_deposition.h)
    _fields_ = [
        ("coordinate", ctypes.c_int32), ("capacity", ctypes.c_int32),
        ("kinetics", ctypes.c_int32), ("sum", ctypes.c_int32),
        ("time_step", c_f64), ("cell_volume", c_f64),
    ]


class ChemistryCfg(ctypes.Structure):  # == sdm_chemistry_cfg (include/sdm_chemistry.h)
    _fields_ = [
        ("n_substep", ctypes.c_int32), ("system_type", ctypes.c_int32), ("sum", ctypes.c_int32),
        ("constants", ctypes.c_int32), ("timestep", c_f64), ("cell_volume", c_f64),
        ("H_min", c_f64), ("H_max", c_f64), ("ionic_strength_threshold", c_f64), ("rtol", c_f64),
    ]


class CondFormulae(ctypes.Structure):  # == sdm_cond_formulae (include/sdm_condensation_formulae.h)
    _fields_ = [("option", ctypes.c_int32 * 10), ("consts", c_f64 * 72)]


class ParcelCfg(ctypes.Structure):  # == sdm_parcel_cfg (include/sdm_parcel.h)
    _fields_ = [
        ("dt", c_f64), ("g_std", c_f64), ("rtol_x", c_f64), ("rtol_thd", c_f64),
        ("dt_min", c_f64), ("dt_max", c_f64), ("RH_rtol", c_f64),
        ("adaptive", ctypes.c_int32), ("fuse", ctypes.c_int32), ("multiplier", ctypes.c_int32),
        ("max_iters", ctypes.c_int32), ("n_clamp_lo", c_i64), ("n_clamp_hi", c_i64),
        ("steps_per_launch", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ]


PARCEL_STATE_FLOATS = ("z", "rhod", "thd", "qv", "T", "p", "RH", "qv_prev", "mass_of_dry_air")
PARCEL_STATE_FIELDS = (*PARCEL_STATE_FLOATS, "n_substeps", "n_activating", "n_deactivating",
                       "n_ripening", "RH_max", "steps_done", "failed_step")
PARCEL_PROFILE_FIELDS = ("z", "rhod", "thd", "qv", "T", "p", "RH", "RH_max", "n_substeps",
                         "n_activating", "n_deactivating", "n_ripening")


class ParcelState(ctypes.Structure):  # == sdm_parcel_state
    _fields_ = [(name, c_ptr) for name in PARCEL_STATE_FIELDS]


class ParcelProfile(ctypes.Structure):  # == sdm_parcel_profile
    _fields_ = [(name, c_ptr) for name in PARCEL_PROFILE_FIELDS]


# include/sdm_parcel_diag.h: SDM_PARCEL_MAX_*, SDM_PARCEL_ATTR_*, SDM_PARCEL_FILTER_*
PARCEL_MAX_MOMENTS, PARCEL_MAX_BINS = 16, 256
PARCEL_ATTRS = {"water mass": 0, "volume": 1, "radius": 2, "dry volume": 3, "dry radius": 4}
PARCEL_FILTERS = {"water mass": 0, "signed water mass": 0, "volume": 1, "dry volume": 2,
                  "wet to critical volume ratio": 3}
PARCEL_DIAG_FIELDS = ("moment_0", "moments", "spectrum", "dv")


class ParcelMomentRequest(ctypes.Structure):  # == sdm_parcel_moment_request
    _fields_ = [
        ("attr", ctypes.c_int32), ("filter_attr", ctypes.c_int32), ("rank", c_f64),
        ("min_x", c_f64), ("max_x", c_f64), ("skip_division_by_m0", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class ParcelRequests(ctypes.Structure):  # == sdm_parcel_requests
    _fields_ = [
        ("n_moments", ctypes.c_int32), ("n_bins", ctypes.c_int32), ("bin_attr", ctypes.c_int32),
        ("reserved", ctypes.c_int32), ("moment", ParcelMomentRequest * PARCEL_MAX_MOMENTS),
        ("edges", c_f64 * (PARCEL_MAX_BINS + 1)),
    ]


class ParcelDiag(ctypes.Structure):  # == sdm_parcel_diag
    _fields_ = [(name, c_ptr) for name in PARCEL_DIAG_FIELDS]


class ParcelChemProfile(ctypes.Structure):  # == sdm_parcel_chem_profile (include/sdm_parcel_chem.h)
    _fields_ = [("mixing_ratio", c_ptr * 6), ("aq_total", c_ptr * 7), ("n_flagged", c_ptr),
                ("dv", c_ptr)]


class ParcelVent(ctypes.Structure):  # == sdm_parcel_vent (include/sdm_parcel_vent.h)
    _fields_ = [
        ("velocity_law", ctypes.c_int32), ("velocity_terms", ctypes.c_int32),
        ("velocity_params", c_ptr), ("gk_a", c_ptr), ("gk_b", c_ptr), ("gk_table_len", c_i64),
        ("gk_factor", c_f64), ("gk_top", c_f64), ("air_density", c_ptr),
        ("air_dynamic_viscosity", c_ptr), ("reynolds_number", c_ptr), ("out_of_table", c_ptr),
    ]


# include/sdm_parcel_ice.h: SDM_PARCEL_ICE_*
PARCEL_ICE_ORDERS = {"freezing_first": 0, "deposition_first": 1}
PARCEL_ICE_STATE_FIELDS = ("a_w_ice", "RH_ice", "rng_offset", "rng_state_inc", "n_exceeded",
                           "freezing_temperature", "immersed_surface_area",
                           "temperature_of_last_freezing")
PARCEL_ICE_PROFILE_FIELDS = ("a_w_ice", "RH_ice", "n_ice", "ice_mass", "n_exceeded", "dv")


class ParcelIceCfg(ctypes.Structure):  # == sdm_parcel_ice_cfg (include/sdm_parcel_ice.h)
    _fields_ = [(name, ctypes.c_int32) for name in (
        "freezing", "deposition", "order", "singular", "immersion_freezing",
        "homogeneous_freezing", "thaw", "j_het", "j_hom", "coordinate", "capacity", "kinetics",
        "sum", "reserved")]


class ParcelIceState(ctypes.Structure):  # == sdm_parcel_ice_state
    _fields_ = [(name, c_ptr) for name in PARCEL_ICE_STATE_FIELDS]


class ParcelIceProfile(ctypes.Structure):  # == sdm_parcel_ice_profile
    _fields_ = [(name, c_ptr) for name in PARCEL_ICE_PROFILE_FIELDS]


# include/sdm_parcel_coal.h: SDM_PARCEL_COAL_*
PARCEL_COAL_MAX_ROWS, PARCEL_COAL_MAX_GRID = 2048, 1024
PARCEL_COAL_EVENT_BOUND, PARCEL_COAL_EVENT_DT_MIN, PARCEL_COAL_OVERFLOW_SHIFT = 0x1, 0x100, 32
PARCEL_COAL_STATE_FIELDS = ("idx", "n_live", "kappa_times_dry_volume", "collision_rate",
                            "collision_rate_deficit", "coalescence_rate", "stats_n_substep",
                            "stats_dt_min", "events", "rng_offset", "rng_state_inc", "gk_a", "gk_b",
                            "velocity_params")
PARCEL_COAL_PROFILE_FIELDS = ("n_live", "n_substeps", "coalescence_rate",
                              "collision_rate_deficit", "dv")


class ParcelCoalState(ctypes.Structure):  # == sdm_parcel_coal_state (include/sdm_parcel_coal.h)
    _fields_ = [(name, c_ptr) for name in PARCEL_COAL_STATE_FIELDS]


class ParcelCoalProfile(ctypes.Structure):  # == sdm_parcel_coal_profile
    _fields_ = [(name, c_ptr) for name in PARCEL_COAL_PROFILE_FIELDS]


# include/sdm_parcel_breakup.h
PARCEL_BREAKUP_STATE_FIELDS = ("breakup_rate", "breakup_rate_deficit", "rng_offset_breakup")
PARCEL_BREAKUP_PROFILE_FIELDS = ("breakup_rate", "breakup_rate_deficit", "n_overflow")


class ParcelBreakupState(ctypes.Structure):  # == sdm_parcel_breakup_state
    _fields_ = [(name, c_ptr) for name in PARCEL_BREAKUP_STATE_FIELDS]


class ParcelBreakupProfile(ctypes.Structure):  # == sdm_parcel_breakup_profile
    _fields_ = [(name, c_ptr) for name in PARCEL_BREAKUP_PROFILE_FIELDS]


class RelaxedVelocityCfg(ctypes.Structure):  # == sdm_relaxed_velocity_cfg
    _fields_ = [
        ("n_sd", c_i64), ("gk_table_len", c_i64), ("dt", c_f64), ("c", c_f64), ("rho_w", c_f64),
        ("gk_factor", c_f64), ("gk_top", c_f64), ("rogers_yau", c_f64 * 5),
        ("constant", ctypes.c_int32), ("law", ctypes.c_int32),
    ]


# ---- header parsing -------------------------------------------------------------------------
_SCALARS = {"int": c_int, "int64_t": c_i64, "uint64_t": c_u64, "double": c_f64,
            "int32_t": ctypes.c_int32}
_ELEMENT = {"double": (np.float64,), "int64_t": (np.int64,), "uint8_t": (np.uint8, np.bool_),
            "uint64_t": (np.uint64,), "int32_t": (np.int32,)}


class Param:  # pylint: disable=too-few-public-methods
    """one C parameter: kind in {ctx, scalar, pointer, host_array, pointer_array}"""

    def __init__(self, text):
        text = " ".join(text.split())
        match = re.match(r"^(.*?)(\w+)(\[\d*\])?$", text)
        self.name = match.group(2)
        ctype = match.group(1).strip()
        self.array_len = None
        if match.group(3):
            digits = match.group(3)[1:-1]
            self.array_len = int(digits) if digits else -1
        self.base = ctype.replace("const", "").replace("*", "").strip()
        stars = ctype.count("*")
        if self.base == "sdm_ctx":
            self.kind = "ctx" if stars == 1 else "pointer"
        elif self.array_len is not None:
            # `double *const moles[7]`: a host array of pointers to columns
            self.kind = "pointer_array" if stars else "host_array"
        elif stars:
            self.kind = "pointer"
        else:
            self.kind = "scalar"

    def convert(self, value, symbol):
        if self.kind == "scalar":
            return _SCALARS[self.base](value)
        if self.kind == "host_array":
            return _host_array(value, self, symbol)
        if self.kind == "pointer_array":
            return _pointer_array(value, self, symbol)
        return _pointer(value, self, symbol)


def _host_array(value, param, symbol):
    if isinstance(value, ctypes.Array):
        return value
    values = [v for v in value]
    if param.array_len not in (None, -1) and len(values) != param.array_len:
        raise ValueError(f"{symbol}: `{param.name}` takes {param.array_len} values, "
                         f"got {len(values)}")
    return (_SCALARS[param.base] * len(values))(*values)


def _pointer_array(value, param, symbol):
    """a host array of column pointers, every column checked like a single pointer parameter"""
    columns = list(value)
    if len(columns) != param.array_len:
        raise ValueError(f"{symbol}: `{param.name}` takes {param.array_len} columns, "
                         f"got {len(columns)}")
    out = (c_ptr * len(columns))()
    for at, column in enumerate(columns):
        if column is None:
            raise ValueError(f"{symbol}: `{param.name}[{at}]` is missing")
        pointer = _pointer(column, param, symbol)
        out[at] = pointer.value if isinstance(pointer, c_ptr) else ctypes.cast(
            pointer, c_ptr).value
    return out


def _pointer(value, param, symbol):
    if value is None:
        return c_ptr(0)
    if isinstance(value, (ctypes._SimpleCData, ctypes.Structure, ctypes.Array)):  # pylint: disable=protected-access
        return ctypes.byref(value)
    if isinstance(value, type(ctypes.byref(c_int()))) or isinstance(value, c_ptr):
        return value
    if isinstance(value, int):
        return c_ptr(value)
    if isinstance(value, (list, tuple)):  # a small host array (e.g. coefficients)
        return (_SCALARS[param.base] * len(value))(*value)
    allowed = _ELEMENT.get(param.base)
    if isinstance(value, np.ndarray):
        if not value.flags["C_CONTIGUOUS"]:
            raise ValueError(f"{symbol}: `{param.name}` is not contiguous")
        if allowed and value.dtype.type not in allowed:
            raise TypeError(f"{symbol}: `{param.name}` is {param.base}*, got {value.dtype}")
        return c_ptr(value.ctypes.data)
    if hasattr(value, "data_ptr"):  # torch tensor
        if not value.is_contiguous():
            raise ValueError(f"{symbol}: `{param.name}` is not contiguous")
        if allowed:
            names = {np.dtype(t).name for t in allowed} | ({"bool"} if np.bool_ in allowed
                                                          else set())
            if str(value.dtype).rsplit(".", maxsplit=1)[-1] not in names:
                raise TypeError(f"{symbol}: `{param.name}` is {param.base}*, got {value.dtype}")
        return c_ptr(value.data_ptr())
    raise TypeError(f"{symbol}: cannot pass {type(value).__name__} as `{param.name}`")


def parse_header(path=HEADER_PATH):
    """{symbol: (return kind, [Param, ...])} for every function the header declares"""
    with open(path, encoding="utf-8") as header:
        text = header.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    table = {}
    for ret, name, params in re.findall(
            r"\b(int|const char \*)\s*(sdm_[A-Za-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = params.strip()
        plist = [] if params in ("", "void") else [Param(p) for p in params.split(",")]
        table[name] = ("str" if "char" in ret else "int", plist)
    return table


def declared_symbols():
    return sorted(parse_header())


class Library:
    """a shared library implementing a header (include/sdm_hip.h unless `header` names another),
    with checked, converting callables"""

    def __init__(self, path, what, header=HEADER_PATH):
        if not os.path.exists(path):
            raise ImportError(f"{path} is missing ({what}); build it with "
                              f"`python -c 'import __graft_entry__ as g; g.build()'`")
        self.path = path
        self.cdll = ctypes.CDLL(path)
        self.signatures = parse_header(header)
        missing = [name for name in self.signatures if not hasattr(self.cdll, name)]
        if missing:
            raise ImportError(f"{path} lacks symbols declared in {os.path.basename(header)}: "
                              f"{missing}")
        for name, (ret, _) in self.signatures.items():
            getattr(self.cdll, name).restype = ctypes.c_char_p if ret == "str" else c_int
        # (declared by sdm_hip.h; the headers of the other paths use it without declaring it)
        self.cdll.sdm_last_error.restype = ctypes.c_char_p

    def last_error(self):
        return self.cdll.sdm_last_error().decode()

    def check(self, code):
        if code != 0:
            raise RuntimeError(f"{os.path.basename(self.path)}: error {code}: "
                               f"{self.last_error()}")

    def invoke(self, symbol, ctx_handle, args):
        """calls `symbol(ctx, *args)`; array / dtype checks first, return code checked after"""
        _, params = self.signatures[symbol]
        expected = [p for p in params if p.kind != "ctx"]
        if len(args) != len(expected):
            raise TypeError(f"{symbol} takes {len(expected)} arguments "
                            f"({', '.join(p.name for p in expected)}), got {len(args)}")
        converted, it = [], iter(args)
        for param in params:
            converted.append(ctx_handle if param.kind == "ctx"
                             else param.convert(next(it), symbol))
        self.check(getattr(self.cdll, symbol)(*converted))


_hip_library = None
_condensation_library = None
_condensation_formulae_library = None
_freezing_library = None
_deposition_library = None
_chemistry_library = None
_seeding_library = None
_relaxed_velocity_library = None
_initialisation_library = None
_parcel_library = None
_parcel_diag_library = None
_parcel_chem_library = None
_parcel_vent_library = None
_parcel_coal_library = None
_parcel_breakup_library = None
_parcel_ice_library = None


def hip_library():
    """libsdm_hip.so (raises ImportError if it is not built: there is no CPU fallback)"""
    global _hip_library  # pylint: disable=global-statement
    if _hip_library is None:
        _hip_library = Library(HIP_LIB_PATH, "the HIP kernels of pysdm_amd")
    return _hip_library


def condensation_library():
    """libsdm_hip.so bound to include/sdm_condensation.h (same file, same contexts)"""
    global _condensation_library  # pylint: disable=global-statement
    if _condensation_library is None:
        _condensation_library = Library(HIP_LIB_PATH, "the HIP kernels of pysdm_amd",
                                        header=CONDENSATION_HEADER_PATH)
    return _condensation_library


def condensation_formulae_library():
    """libsdm_hip.so bound to include/sdm_condensation_formulae.h (same file, same contexts)"""
    global _condensation_formulae_library  # pylint: disable=global-statement
    if _condensation_formulae_library is None:
        _condensation_formulae_library = Library(HIP_LIB_PATH, "the HIP kernels of pysdm_amd",
                                                 header=CONDENSATION_FORMULAE_HEADER_PATH)
    return _condensation_formulae_library


def freezing_library():
    """libsdm_hip.so bound to include/sdm_freezing.h (same file, same contexts)"""
    global _freezing_library  # pylint: disable=global-statement
    if _freezing_library is None:
        _freezing_library = Library(HIP_LIB_PATH, "the HIP kernels of pysdm_amd",
                                    header=FREEZING_HEADER_PATH)
    return _freezing_library


def deposition_library():
    """libsdm_hip.so bound to include/sdm_deposition.h (same file, same contexts)"""
    global _deposition_library  # pylint: disable=global-statement
    if _deposition_library is None:
        _deposition_library = Library(HIP_LIB_PATH, "the HIP kernels of pysdm_amd",
                                      header=DEPOSITION_HEADER_PATH)
    return _deposition_library


def chemistry_library():
    """libsdm_hip.so bound to include/sdm_chemistry.h (same file, same contexts)"""
    global _chemistry_library  # pylint: disable=global-statement
    if _chemistry_library is None:
        _chemistry_library = Library(HIP_LIB_PATH, "the HIP kernels of pysdm_amd",
                                     header=CHEMISTRY_HEADER_PATH)
    return _chemistry_library


def seeding_library():
    """libsdm_hip.so bound to include/sdm_seeding.h (same file, same contexts)"""
    global _seeding_library  # pylint: disable=global-statement
    if _seeding_library is None:
        _seeding_library = Library(HIP_LIB_PATH, "the HIP kernels of pysdm_amd",
                                   header=SEEDING_HEADER_PATH)
    return _seeding_library


def relaxed_velocity_library():
    """libsdm_hip.so bound to include/sdm_relaxed_velocity.h (same file, same contexts)"""
    global _relaxed_velocity_library  # pylint: disable=global-statement
    if _relaxed_velocity_library is None:
        _relaxed_velocity_library = Library(HIP_LIB_PATH, "the HIP kernels of pysdm_amd",
                                            header=RELAXED_VELOCITY_HEADER_PATH)
    return _relaxed_velocity_library


def initialisation_library():
    """libsdm_hip.so bound to include/sdm_initialisation.h (same file, same contexts)"""
    global _initialisation_library  # pylint: disable=global-statement
    if _initialisation_library is None:
        _initialisation_library = Library(HIP_LIB_PATH, "the HIP kernels of pysdm_amd",
                                          header=INITIALISATION_HEADER_PATH)
    return _initialisation_library


def parcel_library():
    """libsdm_hip.so bound to include/sdm_parcel.h (same file, same contexts)"""
    global _parcel_library  # pylint: disable=global-statement
    if _parcel_library is None:
        _parcel_library = Library(HIP_LIB_PATH, "the HIP kernels of pysdm_amd",
                                  header=PARCEL_HEADER_PATH)
    return _parcel_library


def parcel_diag_library():
    """libsdm_hip.so bound to include/sdm_parcel_diag.h (same file, same contexts)"""
    global _parcel_diag_library  # pylint: disable=global-statement
    if _parcel_diag_library is None:
        _parcel_diag_library = Library(HIP_LIB_PATH, "the HIP kernels of pysdm_amd",
                                       header=PARCEL_DIAG_HEADER_PATH)
    return _parcel_diag_library


def parcel_chem_library():
    """libsdm_hip.so bound to include/sdm_parcel_chem.h (same file, same contexts)"""
    global _parcel_chem_library  # pylint: disable=global-statement
    if _parcel_chem_library is None:
        _parcel_chem_library = Library(HIP_LIB_PATH, "the HIP kernels of pysdm_amd",
                                       header=PARCEL_CHEM_HEADER_PATH)
    return _parcel_chem_library


def parcel_vent_library():
    """libsdm_hip.so bound to include/sdm_parcel_vent.h (same file, same contexts)"""
    global _parcel_vent_library  # pylint: disable=global-statement
    if _parcel_vent_library is None:
        _parcel_vent_library = Library(HIP_LIB_PATH, "the HIP kernels of pysdm_amd",
                                       header=PARCEL_VENT_HEADER_PATH)
    return _parcel_vent_library


def parcel_ice_library():
    """libsdm_hip.so bound to include/sdm_parcel_ice.h (same file, same contexts)"""
    global _parcel_ice_library  # pylint: disable=global-statement
    if _parcel_ice_library is None:
        _parcel_ice_library = Library(HIP_LIB_PATH, "the HIP kernels of pysdm_amd",
                                      header=PARCEL_ICE_HEADER_PATH)
    return _parcel_ice_library


def parcel_coal_library():
    """libsdm_hip.so bound to include/sdm_parcel_coal.h (same file, same contexts)"""
    global _parcel_coal_library  # pylint: disable=global-statement
    if _parcel_coal_library is None:
        _parcel_coal_library = Library(HIP_LIB_PATH, "the HIP kernels of pysdm_amd",
                                       header=PARCEL_COAL_HEADER_PATH)
    return _parcel_coal_library


def parcel_breakup_library():
    """libsdm_hip.so bound to include/sdm_parcel_breakup.h (same file, same contexts)"""
    global _parcel_breakup_library  # pylint: disable=global-statement
    if _parcel_breakup_library is None:
        _parcel_breakup_library = Library(HIP_LIB_PATH, "the HIP kernels of pysdm_amd",
                                          header=PARCEL_BREAKUP_HEADER_PATH)
    return _parcel_breakup_library


def pcg64_state_inc(seed):
    """{state_hi, state_lo, inc_hi, inc_lo} of numpy.random.PCG64(seed): NumPy defines the stream
    the reference draws from (PySDM/backends/impl_numba/random.py:16); both libraries reproduce
    it from these four words with jump-ahead"""
    state = np.random.PCG64(seed).state["state"]
    mask = (1 << 64) - 1
    return (state["state"] >> 64, state["state"] & mask, state["inc"] >> 64, state["inc"] & mask)
