"""`Engine`: arrays + calls for one implementation of include/sdm_hip.h.

The host layer of this package (population, runners, PySDM-shaped backend) is written against this
small interface only: allocate / upload / download arrays where the library expects them and call
header symbols by name.  `HipEngine` is the product: torch CUDA tensors (torch is used for device
memory and streams, nothing else) and libsdm_hip.so.  The test suite supplies a second engine over
the CPU oracle (oracle/engine.py, numpy arrays); nothing in this package refers to it.
"""
import ctypes

import numpy as np

from . import abi

FLOAT, INT, BOOL = np.float64, np.int64, np.bool_


class Engine:
    """interface; see HipEngine"""

    name = "abstract"
    library = None
    handle = None
    # the implementation of include/sdm_condensation.h that goes with `library` (same contexts)
    condensation_library = None
    # likewise include/sdm_condensation_formulae.h (the `_f` symbols: non-default formulae)
    condensation_formulae_library = None
    # likewise include/sdm_freezing.h
    freezing_library = None
    # likewise include/sdm_deposition.h
    deposition_library = None
    # likewise include/sdm_chemistry.h
    chemistry_library = None
    # likewise include/sdm_seeding.h
    seeding_library = None
    # likewise include/sdm_relaxed_velocity.h
    relaxed_velocity_library = None
    # likewise include/sdm_initialisation.h
    initialisation_library = None
    # likewise include/sdm_parcel.h
    parcel_library = None
    # likewise include/sdm_parcel_diag.h
    parcel_diag_library = None
    # likewise include/sdm_parcel_chem.h
    parcel_chem_library = None
    # likewise include/sdm_parcel_vent.h
    parcel_vent_library = None
    # likewise include/sdm_parcel_coal.h
    parcel_coal_library = None
    # likewise include/sdm_parcel_breakup.h
    parcel_breakup_library = None
    # likewise include/sdm_parcel_ice.h
    parcel_ice_library = None
    # whether the fused collision step of `library` can take the fall velocity from the
    # "relative fall momentum" row; an engine that cannot must refuse, not ignore the request
    fused_momentum_velocity = False
    # the terminal-velocity laws (keys of pysdm_amd.terminal_velocity.LAWS) the fused collision
    # step of `library` evaluates; a runner refuses the others where a velocity is needed
    fused_velocity_laws = ("GunnKinzer1949",)

    # ---- arrays -----------------------------------------------------------------------------
    def empty(self, shape, dtype):
        raise NotImplementedError

    def upload(self, array):
        """a new library-side array holding a copy of the numpy array"""
        raise NotImplementedError

    def download(self, array):
        """a numpy copy"""
        raise NotImplementedError

    def zeros(self, shape, dtype):
        out = self.empty(shape, dtype)
        self.fill(out, 0)
        return out

    def full(self, shape, dtype, value):
        out = self.empty(shape, dtype)
        self.fill(out, value)
        return out

    @staticmethod
    def fill(array, value):
        array[...] = value

    @staticmethod
    def assign(dst, src):
        dst[...] = src

    @staticmethod
    def size(array):
        return int(np.prod(tuple(array.shape), dtype=np.int64))

    # ---- calls ------------------------------------------------------------------------------
    def call(self, symbol, *args):
        self._before_call()
        self.library.invoke(symbol, self.handle, args)

    def call_condensation(self, symbol, *args):
        """a symbol of include/sdm_condensation.h"""
        if self.condensation_library is None:
            raise NotImplementedError(f"engine `{self.name}` has no condensation library")
        self._before_call()
        self.condensation_library.invoke(symbol, self.handle, args)

    def call_condensation_formulae(self, symbol, *args):
        """a symbol of include/sdm_condensation_formulae.h"""
        if self.condensation_formulae_library is None:
            raise NotImplementedError(
                f"engine `{self.name}` has no library for condensation with non-default formulae")
        self._before_call()
        self.condensation_formulae_library.invoke(symbol, self.handle, args)

    def call_freezing(self, symbol, *args):
        """a symbol of include/sdm_freezing.h"""
        if self.freezing_library is None:
            raise NotImplementedError(f"engine `{self.name}` has no freezing library")
        self._before_call()
        self.freezing_library.invoke(symbol, self.handle, args)

    def call_deposition(self, symbol, *args):
        """a symbol of include/sdm_deposition.h"""
        if self.deposition_library is None:
            raise NotImplementedError(f"engine `{self.name}` has no deposition library")
        self._before_call()
        self.deposition_library.invoke(symbol, self.handle, args)

    def call_chemistry(self, symbol, *args):
        """a symbol of include/sdm_chemistry.h"""
        if self.chemistry_library is None:
            raise NotImplementedError(f"engine `{self.name}` has no chemistry library")
        self._before_call()
        self.chemistry_library.invoke(symbol, self.handle, args)

    def seeding_call(self, symbol, *args):
        """a symbol of include/sdm_seeding.h"""
        if self.seeding_library is None:
            raise NotImplementedError(f"engine `{self.name}` has no seeding library")
        self._before_call()
        self.seeding_library.invoke(symbol, self.handle, args)

    def relaxed_velocity_call(self, symbol, *args):
        """a symbol of include/sdm_relaxed_velocity.h"""
        if self.relaxed_velocity_library is None:
            raise NotImplementedError(f"engine `{self.name}` has no relaxed-velocity library")
        self._before_call()
        self.relaxed_velocity_library.invoke(symbol, self.handle, args)

    def call_initialisation(self, symbol, *args):
        """a symbol of include/sdm_initialisation.h"""
        if self.initialisation_library is None:
            raise NotImplementedError(f"engine `{self.name}` has no initialisation library")
        self._before_call()
        self.initialisation_library.invoke(symbol, self.handle, args)

    def call_parcel(self, symbol, *args):
        """a symbol of include/sdm_parcel.h"""
        if self.parcel_library is None:
            raise NotImplementedError(f"engine `{self.name}` has no parcel library")
        self._before_call()
        self.parcel_library.invoke(symbol, self.handle, args)

    def call_parcel_diag(self, symbol, *args):
        """a symbol of include/sdm_parcel_diag.h"""
        if self.parcel_diag_library is None:
            raise NotImplementedError(f"engine `{self.name}` has no parcel-diagnostics library")
        self._before_call()
        self.parcel_diag_library.invoke(symbol, self.handle, args)

    def call_parcel_chem(self, symbol, *args):
        """a symbol of include/sdm_parcel_chem.h"""
        if self.parcel_chem_library is None:
            raise NotImplementedError(
                f"engine `{self.name}` has no library for the parcel with aqueous chemistry")
        self._before_call()
        self.parcel_chem_library.invoke(symbol, self.handle, args)

    def call_parcel_vent(self, symbol, *args):
        """a symbol of include/sdm_parcel_vent.h"""
        if self.parcel_vent_library is None:
            raise NotImplementedError(
                f"engine `{self.name}` has no library for the ventilated parcel")
        self._before_call()
        self.parcel_vent_library.invoke(symbol, self.handle, args)

    def call_parcel_coal(self, symbol, *args):
        """a symbol of include/sdm_parcel_coal.h"""
        if self.parcel_coal_library is None:
            raise NotImplementedError(
                f"engine `{self.name}` has no library for the parcel with coalescence")
        self._before_call()
        self.parcel_coal_library.invoke(symbol, self.handle, args)

    def call_parcel_breakup(self, symbol, *args):
        """a symbol of include/sdm_parcel_breakup.h"""
        if self.parcel_breakup_library is None:
            raise NotImplementedError(
                f"engine `{self.name}` has no library for the parcel with breakup")
        self._before_call()
        self.parcel_breakup_library.invoke(symbol, self.handle, args)

    def call_parcel_ice(self, symbol, *args):
        """a symbol of include/sdm_parcel_ice.h"""
        if self.parcel_ice_library is None:
            raise NotImplementedError(
                f"engine `{self.name}` has no library for the mixed-phase parcel")
        self._before_call()
        self.parcel_ice_library.invoke(symbol, self.handle, args)

    def _before_call(self):
        pass

    def synchronize(self):
        self.call("sdm_ctx_synchronize")

    def scalar_out(self, symbol, ctype, *args):
        """for symbols whose last parameter is a host out-pointer: returns its value"""
        out = ctype()
        self.call(symbol, *args, out)
        return out.value


class HipEngine(Engine):
    """one sdm_ctx per process and device; follows torch's current stream"""

    name = "hip"
    # fused.hip reads the velocity from the momentum row (sdm_step_cfg.velocity_source)
    fused_momentum_velocity = True
    # fused.hip: sdm_step_cfg.velocity_law
    fused_velocity_laws = ("GunnKinzer1949", "RogersYau", "PowerSeries")
    _instances = {}

    def __init__(self, device_index):
        import torch  # pylint: disable=import-outside-toplevel

        self.torch = torch
        self.library = abi.hip_library()
        self.condensation_library = abi.condensation_library()
        self.condensation_formulae_library = abi.condensation_formulae_library()
        self.freezing_library = abi.freezing_library()
        self.deposition_library = abi.deposition_library()
        self.chemistry_library = abi.chemistry_library()
        self.seeding_library = abi.seeding_library()
        self.relaxed_velocity_library = abi.relaxed_velocity_library()
        self.initialisation_library = abi.initialisation_library()
        self.parcel_library = abi.parcel_library()
        self.parcel_diag_library = abi.parcel_diag_library()
        self.parcel_chem_library = abi.parcel_chem_library()
        self.parcel_vent_library = abi.parcel_vent_library()
        self.parcel_coal_library = abi.parcel_coal_library()
        self.parcel_breakup_library = abi.parcel_breakup_library()
        self.parcel_ice_library = abi.parcel_ice_library()
        self.handle = abi.c_ptr()
        self.library.check(self.library.cdll.sdm_ctx_create(ctypes.byref(self.handle),
                                                            abi.c_int(device_index)))
        self.device = torch.device("cuda", device_index)
        self._stream = None
        self._dtype = {FLOAT: torch.float64, INT: torch.int64, BOOL: torch.bool,
                       np.uint8: torch.uint8}

    @classmethod
    def get(cls, device_index=None):
        import torch  # pylint: disable=import-outside-toplevel

        if not torch.cuda.is_available():
            raise RuntimeError("pysdm_amd needs a GPU (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        if device_index is None:
            device_index = torch.cuda.current_device()
        if device_index not in cls._instances:
            cls._instances[device_index] = cls(device_index)
        return cls._instances[device_index]

    def _before_call(self):
        stream = self.torch.cuda.current_stream(self.device).cuda_stream
        if stream != self._stream:
            self.library.invoke("sdm_ctx_set_stream", self.handle, (stream,))
            self._stream = stream

    def empty(self, shape, dtype):
        return self.torch.empty(shape, dtype=self._dtype[np.dtype(dtype).type],
                                device=self.device)

    def upload(self, array):
        # (a writable, contiguous host copy: torch refuses to wrap read-only arrays quietly - the
        # arrays of an .npz file are read-only)
        return self.torch.from_numpy(np.require(array, requirements=["C", "W"])).to(self.device)

    @staticmethod
    def download(array):
        return array.detach().cpu().numpy()
