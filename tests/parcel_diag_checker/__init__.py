"""TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_parcel_diag.h.

`ParcelDiagCheckerEngine` is the checker engine of tests/parcel_checker with
tests/parcel_diag_checker/parcel_diag_checker.c as its parcel-diagnostics library, and
`ParcelDiagCheckerBackend` the PySDM-shaped class bound to it.  The shared object links against
the parcel checker (whose `sdm_parcel_run` it calls one step at a time) and the two condensation
checkers, and is compiled after them by __graft_entry__.build() with the compiler and flags of
the oracle; nothing under pysdm_amd/ imports this package.
"""
import os

from pysdm_amd import abi
from pysdm_amd.backends.pysdm_shaped import backend_class_for
from tests.parcel_checker import ParcelCheckerEngine

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "parcel_diag_checker.c")
LIB_PATH = os.path.join(HERE, "libparcel_diag_checker.so")


class ParcelDiagCheckerEngine(ParcelCheckerEngine):
    name = "parcel_diag_checker"
    _instances = {}

    def __init__(self, threads=1):
        super().__init__(threads)
        self.parcel_diag_library = abi.Library(
            LIB_PATH, "the CPU checker of the parcel's diagnostics",
            header=abi.PARCEL_DIAG_HEADER_PATH)


ParcelDiagCheckerBackend = backend_class_for(
    ParcelDiagCheckerEngine.get, "ParcelDiagCheckerBackend",
    doc="PySDM-shaped backend over the CPU oracle and the checkers of every path, the parcel's "
        "diagnostics included")
