"""TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_condensation.h.

`CheckerEngine` is the oracle engine (oracle/engine.py: numpy arrays, the serial C restatement of
include/sdm_hip.h) with tests/checker/condensation_checker.c as its condensation library, and
`CheckerBackend` the PySDM-shaped class (pysdm_amd/backends/pysdm_shaped.py, the very class `HIP`
is) bound to it.  The shared object is compiled by __graft_entry__.build() with the compiler and
flags of the oracle; nothing under pysdm_amd/ imports this package.
"""
import os

from oracle.engine import OracleEngine
from pysdm_amd import abi
from pysdm_amd.backends.pysdm_shaped import backend_class_for

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "condensation_checker.c")
LIB_PATH = os.path.join(HERE, "libcondensation_checker.so")


class CheckerEngine(OracleEngine):
    name = "checker"
    _instances = {}

    def __init__(self, threads=1):
        super().__init__(threads)
        self.condensation_library = abi.Library(
            LIB_PATH, "the CPU checker of the condensation path",
            header=abi.CONDENSATION_HEADER_PATH)


CheckerBackend = backend_class_for(
    CheckerEngine.get, "CheckerBackend",
    doc="PySDM-shaped backend over the CPU oracle and the condensation checker")
