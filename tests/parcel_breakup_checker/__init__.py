"""TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_parcel_breakup.h.

`ParcelBreakupCheckerEngine` is the checker engine of tests/parcel_coal_checker with
tests/parcel_breakup_checker/parcel_breakup_checker.c as its parcel-with-breakup library, and
`ParcelBreakupCheckerBackend` the PySDM-shaped class bound to it.  The shared object links against
the parcel checker and the CPU oracle (it loops over `sdm_parcel_run` and `sdm_collision_step` and
restates neither the solver nor the collisions) and is compiled after them by
__graft_entry__.build() with the compiler and flags of the oracle; nothing under pysdm_amd/
imports this package.
"""
import os

from pysdm_amd import abi
from pysdm_amd.backends.pysdm_shaped import backend_class_for
from tests.parcel_coal_checker import ParcelCoalCheckerEngine

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "parcel_breakup_checker.c")
LIB_PATH = os.path.join(HERE, "libparcel_breakup_checker.so")


class ParcelBreakupCheckerEngine(ParcelCoalCheckerEngine):
    name = "parcel_breakup_checker"
    _instances = {}

    def __init__(self, threads=1):
        super().__init__(threads)
        self.parcel_breakup_library = abi.Library(
            LIB_PATH, "the CPU checker of the parcel with breakup",
            header=abi.PARCEL_BREAKUP_HEADER_PATH)


ParcelBreakupCheckerBackend = backend_class_for(
    ParcelBreakupCheckerEngine.get, "ParcelBreakupCheckerBackend",
    doc="PySDM-shaped backend over the CPU oracle and the checkers of every path, the parcel "
        "with breakup included")
