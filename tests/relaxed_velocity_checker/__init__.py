"""TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_relaxed_velocity.h.

`RelaxedVelocityCheckerEngine` is the checker engine of tests/seeding_checker (the CPU oracle with
the checkers of the other paths) with tests/relaxed_velocity_checker/relaxed_velocity_checker.c as
its relaxed-velocity library, and `RelaxedVelocityCheckerBackend` the PySDM-shaped class
(pysdm_amd/backends/pysdm_shaped.py, the very class `HIP` is) bound to it.  The shared object is
compiled by __graft_entry__.build() with the compiler and flags of the oracle; nothing under
pysdm_amd/ imports this package.
"""
import os

from pysdm_amd import abi
from pysdm_amd.backends.pysdm_shaped import backend_class_for
from tests.seeding_checker import SeedingCheckerEngine

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "relaxed_velocity_checker.c")
LIB_PATH = os.path.join(HERE, "librelaxed_velocity_checker.so")


class RelaxedVelocityCheckerEngine(SeedingCheckerEngine):
    name = "relaxed_velocity_checker"
    _instances = {}

    def __init__(self, threads=1):
        super().__init__(threads)
        self.relaxed_velocity_library = abi.Library(
            LIB_PATH, "the CPU checker of the relaxed-velocity path",
            header=abi.RELAXED_VELOCITY_HEADER_PATH)


RelaxedVelocityCheckerBackend = backend_class_for(
    RelaxedVelocityCheckerEngine.get, "RelaxedVelocityCheckerBackend",
    doc="PySDM-shaped backend over the CPU oracle and the checkers of the condensation, freezing, "
        "deposition, chemistry, seeding and relaxed-velocity paths")
