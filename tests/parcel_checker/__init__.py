"""TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_parcel.h.

`ParcelCheckerEngine` is the checker engine of tests/initialisation_checker (the CPU oracle with
the checkers of the other paths) with tests/parcel_checker/parcel_checker.c as its parcel library,
and `ParcelCheckerBackend` the PySDM-shaped class (pysdm_amd/backends/pysdm_shaped.py, the very
class `HIP` is) bound to it.  The shared object links against the two condensation checkers and is
compiled after them by __graft_entry__.build() with the compiler and flags of the oracle; nothing
under pysdm_amd/ imports this package.
"""
import os

from pysdm_amd import abi
from pysdm_amd.backends.pysdm_shaped import backend_class_for
from tests.condensation_formulae_checker import LIB_PATH as FORMULAE_LIB_PATH
from tests.initialisation_checker import InitialisationCheckerEngine

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "parcel_checker.c")
LIB_PATH = os.path.join(HERE, "libparcel_checker.so")


class ParcelCheckerEngine(InitialisationCheckerEngine):
    name = "parcel_checker"
    _instances = {}

    def __init__(self, threads=1):
        super().__init__(threads)
        # (the chain this engine extends branches off before the checker of the `_f` symbols,
        # which the parcel's stage route calls and the parcel checker links against)
        self.condensation_formulae_library = abi.Library(
            FORMULAE_LIB_PATH, "the CPU checker of the condensation path with non-default formulae",
            header=abi.CONDENSATION_FORMULAE_HEADER_PATH)
        self.parcel_library = abi.Library(
            LIB_PATH, "the CPU checker of the parcel path", header=abi.PARCEL_HEADER_PATH)


ParcelCheckerBackend = backend_class_for(
    ParcelCheckerEngine.get, "ParcelCheckerBackend",
    doc="PySDM-shaped backend over the CPU oracle and the checkers of the condensation, freezing, "
        "deposition, chemistry, seeding, relaxed-velocity, initialisation and parcel paths")
