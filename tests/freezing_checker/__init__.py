"""TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_freezing.h.

`FreezingCheckerEngine` is the checker engine of tests/checker (the CPU oracle with the
condensation checker) with tests/freezing_checker/freezing_checker.c as its freezing library, and
`FreezingCheckerBackend` the PySDM-shaped class (pysdm_amd/backends/pysdm_shaped.py, the very
class `HIP` is) bound to it.  The shared object is compiled by __graft_entry__.build() with the
compiler and flags of the oracle; nothing under pysdm_amd/ imports this package.
"""
import os

from pysdm_amd import abi
from pysdm_amd.backends.pysdm_shaped import backend_class_for
from tests.checker import CheckerEngine

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "freezing_checker.c")
LIB_PATH = os.path.join(HERE, "libfreezing_checker.so")


class FreezingCheckerEngine(CheckerEngine):
    name = "freezing_checker"
    _instances = {}

    def __init__(self, threads=1):
        super().__init__(threads)
        self.freezing_library = abi.Library(
            LIB_PATH, "the CPU checker of the freezing path", header=abi.FREEZING_HEADER_PATH)


FreezingCheckerBackend = backend_class_for(
    FreezingCheckerEngine.get, "FreezingCheckerBackend",
    doc="PySDM-shaped backend over the CPU oracle and the condensation and freezing checkers")
