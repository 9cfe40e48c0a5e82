"""TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_parcel_chem.h.

`ParcelChemCheckerEngine` is the checker engine of tests/parcel_diag_checker with
tests/parcel_chem_checker/parcel_chem_checker.c as its parcel-with-chemistry library, and
`ParcelChemCheckerBackend` the PySDM-shaped class bound to it.  The shared object links against
the parcel, chemistry and parcel-diagnostics checkers (it loops over their symbols and restates
neither solver) and is compiled after them by __graft_entry__.build() with the compiler and flags
of the oracle; nothing under pysdm_amd/ imports this package.
"""
import os

from pysdm_amd import abi
from pysdm_amd.backends.pysdm_shaped import backend_class_for
from tests.parcel_diag_checker import ParcelDiagCheckerEngine

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "parcel_chem_checker.c")
LIB_PATH = os.path.join(HERE, "libparcel_chem_checker.so")


class ParcelChemCheckerEngine(ParcelDiagCheckerEngine):
    name = "parcel_chem_checker"
    _instances = {}

    def __init__(self, threads=1):
        super().__init__(threads)
        self.parcel_chem_library = abi.Library(
            LIB_PATH, "the CPU checker of the parcel with aqueous chemistry",
            header=abi.PARCEL_CHEM_HEADER_PATH)


ParcelChemCheckerBackend = backend_class_for(
    ParcelChemCheckerEngine.get, "ParcelChemCheckerBackend",
    doc="PySDM-shaped backend over the CPU oracle and the checkers of every path, the parcel "
        "with aqueous chemistry included")
