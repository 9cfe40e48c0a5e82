"""TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_parcel_vent.h.

`ParcelVentCheckerEngine` is the checker engine of tests/parcel_diag_checker with
tests/parcel_vent_checker/parcel_vent_checker.c as its ventilated-parcel library, and
`ParcelVentCheckerBackend` the PySDM-shaped class bound to it.  The shared object links against
the CPU oracle (radius and the fall-velocity laws), the two condensation checkers (the air's
density and viscosity, the Reynolds number, the critical volume, the solver) and the
parcel-diagnostics checker; it loops over their stage symbols and restates no solver.  It is
compiled after them by __graft_entry__.build() with the compiler and flags of the oracle; nothing
under pysdm_amd/ imports this package.
"""
import os

from pysdm_amd import abi
from pysdm_amd.backends.pysdm_shaped import backend_class_for
from tests.parcel_diag_checker import ParcelDiagCheckerEngine

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "parcel_vent_checker.c")
LIB_PATH = os.path.join(HERE, "libparcel_vent_checker.so")


class ParcelVentCheckerEngine(ParcelDiagCheckerEngine):
    name = "parcel_vent_checker"
    _instances = {}

    def __init__(self, threads=1):
        super().__init__(threads)
        self.parcel_vent_library = abi.Library(
            LIB_PATH, "the CPU checker of the ventilated parcel",
            header=abi.PARCEL_VENT_HEADER_PATH)


ParcelVentCheckerBackend = backend_class_for(
    ParcelVentCheckerEngine.get, "ParcelVentCheckerBackend",
    doc="PySDM-shaped backend over the CPU oracle and the checkers of every path, the ventilated "
        "parcel included")
