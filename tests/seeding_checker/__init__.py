"""TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_seeding.h.

`SeedingCheckerEngine` is the checker engine of tests/chemistry_checker (the CPU oracle with the
condensation, freezing, deposition and chemistry checkers) with
tests/seeding_checker/seeding_checker.c as its seeding library, and `SeedingCheckerBackend` the
PySDM-shaped class (pysdm_amd/backends/pysdm_shaped.py, the very class `HIP` is) bound to it.  The
shared object is compiled by __graft_entry__.build() with the compiler and flags of the oracle;
nothing under pysdm_amd/ imports this package.
"""
import os

from pysdm_amd import abi
from pysdm_amd.backends.pysdm_shaped import backend_class_for
from tests.chemistry_checker import ChemistryCheckerEngine

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "seeding_checker.c")
LIB_PATH = os.path.join(HERE, "libseeding_checker.so")


class SeedingCheckerEngine(ChemistryCheckerEngine):
    name = "seeding_checker"
    _instances = {}

    def __init__(self, threads=1):
        super().__init__(threads)
        self.seeding_library = abi.Library(
            LIB_PATH, "the CPU checker of the seeding path", header=abi.SEEDING_HEADER_PATH)


SeedingCheckerBackend = backend_class_for(
    SeedingCheckerEngine.get, "SeedingCheckerBackend",
    doc="PySDM-shaped backend over the CPU oracle and the condensation, freezing, deposition, "
        "chemistry and seeding checkers")
