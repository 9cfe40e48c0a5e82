"""TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_condensation_formulae.h.

`CheckerEngine` is the engine of tests/checker (the oracle plus the default formulae's condensation
checker) with tests/condensation_formulae_checker/condensation_formulae_checker.c as its library
for the `_f` symbols, and `CheckerBackend` the PySDM-shaped class (pysdm_amd/backends/
pysdm_shaped.py, the very class `HIP` is) bound to it.  The shared object is compiled by
__graft_entry__.build() with the compiler and flags of the oracle; nothing under pysdm_amd/ imports
this package.
"""
import os

from pysdm_amd import abi
from pysdm_amd.backends.pysdm_shaped import backend_class_for
from tests.checker import CheckerEngine as _DefaultCheckerEngine

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "condensation_formulae_checker.c")
LIB_PATH = os.path.join(HERE, "libcondensation_formulae_checker.so")


class CheckerEngine(_DefaultCheckerEngine):
    name = "formulae-checker"
    _instances = {}

    def __init__(self, threads=1):
        super().__init__(threads)
        self.condensation_formulae_library = abi.Library(
            LIB_PATH, "the CPU checker of condensation with non-default formulae",
            header=abi.CONDENSATION_FORMULAE_HEADER_PATH)


CheckerBackend = backend_class_for(
    CheckerEngine.get, "FormulaeCheckerBackend",
    doc="PySDM-shaped backend over the CPU oracle and the two condensation checkers")
