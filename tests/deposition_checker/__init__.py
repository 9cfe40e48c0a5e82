"""TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_deposition.h.

`DepositionCheckerEngine` is the checker engine of tests/freezing_checker (the CPU oracle with the
condensation and freezing checkers, which `AmbientColumns(..., mixed_phase=True)` needs) with
tests/deposition_checker/deposition_checker.c as its deposition library, and
`DepositionCheckerBackend` the PySDM-shaped class (pysdm_amd/backends/pysdm_shaped.py, the very
class `HIP` is) bound to it.  The shared object is compiled by __graft_entry__.build() with the
compiler and flags of the oracle; nothing under pysdm_amd/ imports this package.
"""
import os

from pysdm_amd import abi
from pysdm_amd.backends.pysdm_shaped import backend_class_for
from tests.freezing_checker import FreezingCheckerEngine

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "deposition_checker.c")
LIB_PATH = os.path.join(HERE, "libdeposition_checker.so")


class DepositionCheckerEngine(FreezingCheckerEngine):
    name = "deposition_checker"
    _instances = {}

    def __init__(self, threads=1):
        super().__init__(threads)
        self.deposition_library = abi.Library(
            LIB_PATH, "the CPU checker of the deposition path",
            header=abi.DEPOSITION_HEADER_PATH)


DepositionCheckerBackend = backend_class_for(
    DepositionCheckerEngine.get, "DepositionCheckerBackend",
    doc="PySDM-shaped backend over the CPU oracle and the condensation, freezing and deposition "
        "checkers")
