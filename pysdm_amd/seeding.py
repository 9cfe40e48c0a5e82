"""Super-droplet seeding on the library (include/sdm_seeding.h): injection into free slots.

`SeedingRunner` is PySDM's `Seeding` dynamic (PySDM/dynamics/seeding.py) with what
`Particulator.seeding` does around the backend call (PySDM/particulator.py:447-499), over a
`Population`: a reservoir of seeds (multiplicities and one value per extensive row), a rate
function `injection_rate(time) -> number of super-droplets to inject at this step`, and per
injecting step a shuffle of the seed index (reservoirs of more than one seed; the NumPy-PCG64
stream of `seed`, one number per seed, as PySDM's `Random`), the injection into the first free
slots in slot order, the identity permutation and the removal of what has multiplicity 0.

A free slot is a slot of multiplicity 0: one that was created unused (NaN multiplicity, see
`Population`) or emptied by coalescence.  As in the reference a seed is not placed in space: the
slot keeps its cell id and its position, so the seed appears where the previous owner was.

Routes: "fused" - one `sdm_seeding_step` per injecting step - and "stages" - uniforms,
`sdm_shuffle_global`, `sdm_seeding`, `sdm_identity_index`, `sdm_remove_zero_n_or_flagged`.  Same
results to the bit.  A step whose rate is 0 launches nothing and draws nothing.
"""
import ctypes

import numpy as np

from .abi import pcg64_state_inc
from .engine import FLOAT, INT
from .population import to_integer_multiplicities

NO_SLOTS = ("No available seeds to inject. Please provide particles with nan filled "
            "attributes.")
NO_SPACE = "Trying to inject more super particles than space available."
# (the reference's text, the indentation behind its line continuation included:
# particulator.py:467-470)
SAME_ATTRIBUTES = ("Trying to inject multiple super particles with the same attributes. "
                   + " " * 16 + "Instead increase multiplicity of injected particles.")
ROUTES = ("fused", "stages")
STATUS_FREE, STATUS_INJECTED, STATUS_BAD_SEED, STATUS_WORDS = 0, 1, 2, 4
# in the message of a `sdm_seeding_step` that refused on the device (SDM_E_STATE): by then the
# seed index has been shuffled, i.e. the uniform numbers of this step are spent
REFUSED_ON_DEVICE = "nothing injected"


def check_counts(n_sd, live, n_seeds, number_to_inject):
    """the three refusals of `Particulator.seeding`, in its order"""
    n_null = int(n_sd) - int(live)
    if n_null == 0:
        raise ValueError(NO_SLOTS)
    if number_to_inject > n_null:
        raise ValueError(NO_SPACE)
    if number_to_inject > n_seeds:
        raise ValueError(SAME_ATTRIBUTES)


def shuffled_before_failing(error):
    """True if the failed `sdm_seeding_step` behind `error` got as far as its shuffle (a refusal on
    the device; an argument error returns before anything is launched)"""
    return REFUSED_ON_DEVICE in str(error)


def raise_if_refused(status, number_to_inject):
    """`status`: the host copy of sdm_seeding's status words.  The library stores nothing when it
    finds fewer free slots than asked for (the reference asserts after having written)"""
    if int(status[STATUS_INJECTED]) == int(number_to_inject):
        return
    if int(status[STATUS_BAD_SEED]):
        raise ValueError(f"seeding: {int(status[STATUS_BAD_SEED])} seed indices outside the "
                         "reservoir; nothing was injected")
    raise ValueError(f"seeding: {int(number_to_inject)} super particles to inject but "
                     f"{int(status[STATUS_FREE])} free slots; nothing was injected")


class SeedingRunner:  # pylint: disable=too-many-instance-attributes
    """`Seeding(super_droplet_injection_rate=injection_rate, seeded_particle_multiplicity=
    multiplicity, seeded_particle_extensive_attributes=extensive)` on `population`; `extensive`
    names its rows as `population.rows` does, in the same order."""

    def __init__(self, population, *, multiplicity, extensive, injection_rate, dt, seed,
                 route="fused"):
        if route not in ROUTES:
            raise ValueError(f"route={route!r}: one of {ROUTES}")
        if tuple(population.rows) != tuple(extensive.keys()):  # seeding.py:36-43
            raise ValueError(f"extensive attributes ({tuple(extensive.keys())}) do not match "
                             f"those used in the population ({tuple(population.rows)})")
        self.population, self.route = population, route
        self.injection_rate, self.dt = injection_rate, float(dt)
        eng = self.engine = population.engine
        counts = to_integer_multiplicities(np.asarray(multiplicity))
        self.n_seeds = int(counts.shape[0])
        rows = np.asarray(list(extensive.values()), dtype=float).reshape(len(extensive),
                                                                        self.n_seeds)
        self.index = eng.upload(np.arange(self.n_seeds, dtype=np.int64))
        self.seed_multiplicity = eng.upload(np.ascontiguousarray(counts, dtype=np.int64))
        self.seed_extensive = eng.upload(np.ascontiguousarray(rows))
        # a reservoir of one seed never creates a stream (seeding.py:48-51)
        self.state_inc = pcg64_state_inc(int(seed)) if self.n_seeds > 1 else None
        self.rng_offset = 0
        self.u01 = eng.empty(self.n_seeds, FLOAT) if self.n_seeds > 1 else None
        self.status = eng.zeros(STATUS_WORDS, INT)
        self.n_steps = 0
        self.n_injections = 0

    def step(self):
        """one `Seeding.__call__` at time n_steps * dt"""
        number = self.injection_rate(self.n_steps * self.dt)
        if number > 0:
            self.inject(int(number))
        self.n_steps += 1

    def run(self, n_steps):
        for _ in range(int(n_steps)):
            self.step()

    def inject(self, number):
        pop, eng = self.population, self.engine
        check_counts(pop.n_sd, self._live(), self.n_seeds, number)
        n_attr = int(pop.extensive.shape[0])
        # (the stream position moves with the shuffle, also where the device then refuses - which
        # the check above leaves to states whose bookkeeping is wrong: index and stream stay together)
        if self.route == "fused":
            new_length = ctypes.c_int64(-1)
            try:
                eng.seeding_call(
                    "sdm_seeding_step", pop.perm, pop.multiplicity, pop.extensive, n_attr,
                    pop.n_sd, self.index, self.seed_multiplicity, self.seed_extensive,
                    self.n_seeds, number, int(self.state_inc is not None),
                    self.state_inc or (0, 0, 0, 0), self.rng_offset, new_length)
            except RuntimeError as error:
                if self.state_inc is not None and shuffled_before_failing(error):
                    self.rng_offset += self.n_seeds
                raise
            if self.state_inc is not None:
                self.rng_offset += self.n_seeds
            live = int(new_length.value)
        else:
            if self.state_inc is not None:
                eng.call("sdm_pcg64_uniform", self.u01, self.n_seeds, self.state_inc,
                         self.rng_offset)
                eng.call("sdm_shuffle_global", self.index, self.n_seeds, self.u01)
                self.rng_offset += self.n_seeds
            eng.seeding_call(
                "sdm_seeding", pop.perm, pop.multiplicity, pop.extensive, n_attr, pop.n_sd,
                self.index, self.seed_multiplicity, self.seed_extensive, self.n_seeds, number,
                self.status)
            raise_if_refused(eng.download(self.status), number)
            eng.call("sdm_identity_index", pop.perm, pop.n_sd)
            live = eng.scalar_out("sdm_remove_zero_n_or_flagged", ctypes.c_int64,
                                  pop.multiplicity, pop.perm, pop.n_sd, pop.n_sd)
        self.n_injections += 1
        pop.live = pop.working = live
        pop.ordered = False
        eng.fill(pop.healthy, 1)
        pop.touch_state()  # (also host_dirty: the next fused collision step starts from this view)

    def _live(self):
        """the number of live super-droplets, the dead of a collision step compacted away first
        (the reference's `super_droplet_count` asserts a healthy state)"""
        pop = self.population
        pop.refresh_bookkeeping()
        pop.compact()
        return pop.live

    def seed_index(self):
        """host copy of the (shuffled) seed index"""
        return self.engine.download(self.index)
