"""TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_parcel_ice.h.

`ParcelIceCheckerEngine` is the checker engine of tests/parcel_diag_checker (which carries the
freezing and deposition checkers too) with tests/parcel_ice_checker/parcel_ice_checker.c as its
mixed-phase-parcel library.  The shared object links against the two condensation checkers, the
freezing checker and the deposition checker; it loops over their stage symbols and restates no
solver, no row arithmetic and no generator.  It is compiled after them by __graft_entry__.build()
with the compiler and flags of the oracle; nothing under pysdm_amd/ imports this package.
"""
import os

from pysdm_amd import abi
from tests.parcel_diag_checker import ParcelDiagCheckerEngine

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "parcel_ice_checker.c")
LIB_PATH = os.path.join(HERE, "libparcel_ice_checker.so")


class ParcelIceCheckerEngine(ParcelDiagCheckerEngine):
    name = "parcel_ice_checker"
    _instances = {}

    def __init__(self, threads=1):
        super().__init__(threads)
        self.parcel_ice_library = abi.Library(
            LIB_PATH, "the CPU checker of the mixed-phase parcel",
            header=abi.PARCEL_ICE_HEADER_PATH)
