"""TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_chemistry.h.

`ChemistryCheckerEngine` is the checker engine of tests/deposition_checker (the CPU oracle with
the condensation, freezing and deposition checkers) with
tests/chemistry_checker/chemistry_checker.c as its chemistry library, and
`ChemistryCheckerBackend` the PySDM-shaped class (pysdm_amd/backends/pysdm_shaped.py, the very
class `HIP` is) bound to it.  The shared object is compiled by __graft_entry__.build() with the
compiler and flags of the oracle; nothing under pysdm_amd/ imports this package.
"""
import os

from pysdm_amd import abi
from pysdm_amd.backends.pysdm_shaped import backend_class_for
from tests.deposition_checker import DepositionCheckerEngine

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "chemistry_checker.c")
LIB_PATH = os.path.join(HERE, "libchemistry_checker.so")


class ChemistryCheckerEngine(DepositionCheckerEngine):
    name = "chemistry_checker"
    _instances = {}

    def __init__(self, threads=1):
        super().__init__(threads)
        self.chemistry_library = abi.Library(
            LIB_PATH, "the CPU checker of the chemistry path", header=abi.CHEMISTRY_HEADER_PATH)


ChemistryCheckerBackend = backend_class_for(
    ChemistryCheckerEngine.get, "ChemistryCheckerBackend",
    doc="PySDM-shaped backend over the CPU oracle and the condensation, freezing, deposition and "
        "chemistry checkers")
