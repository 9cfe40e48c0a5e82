"""TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_initialisation.h.

`InitialisationCheckerEngine` is the checker engine of tests/relaxed_velocity_checker (the CPU
oracle with the checkers of the other paths) with tests/initialisation_checker/
initialisation_checker.c as its initialisation library, and `InitialisationCheckerBackend` the
PySDM-shaped class (pysdm_amd/backends/pysdm_shaped.py, the very class `HIP` is) bound to it.  The
shared object is compiled by __graft_entry__.build() with the compiler and flags of the oracle;
nothing under pysdm_amd/ imports this package.
"""
import os

from pysdm_amd import abi
from pysdm_amd.backends.pysdm_shaped import backend_class_for
from tests.relaxed_velocity_checker import RelaxedVelocityCheckerEngine

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "initialisation_checker.c")
LIB_PATH = os.path.join(HERE, "libinitialisation_checker.so")


class InitialisationCheckerEngine(RelaxedVelocityCheckerEngine):
    name = "initialisation_checker"
    _instances = {}

    def __init__(self, threads=1):
        super().__init__(threads)
        self.initialisation_library = abi.Library(
            LIB_PATH, "the CPU checker of the initialisation path",
            header=abi.INITIALISATION_HEADER_PATH)


InitialisationCheckerBackend = backend_class_for(
    InitialisationCheckerEngine.get, "InitialisationCheckerBackend",
    doc="PySDM-shaped backend over the CPU oracle and the checkers of the condensation, freezing, "
        "deposition, chemistry, seeding, relaxed-velocity and initialisation paths")
